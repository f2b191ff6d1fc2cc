"""Builds the two native libraries of the package in-tree (pose2mesh_release_amd/lib/):

  libp2m_hip.so   HIP kernels + C ABI (include/p2m.h), cross-compiled for gfx950 with hipcc
  libp2m_host.so  CPU-only helpers for graph preparation (g++)

`python -m pose2mesh_release_amd.build` or __graft_entry__.build() runs this; a rebuild happens
only when a source is newer than the library.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
HIP_SOURCES = ["capi.hip", "basis.hip", "gemm_planes.hip", "gemm_tn.hip", "weights.hip", "amax.hip", "bn.hip", "optim.hip",
               "loss.hip", "chebtile.hip", "posenet.hip", "eval.hip", "body.hip", "body_bwd.hip", "fscore.hip", "sample.hip",
               "render.hip", "camfit.hip", "video.hip", "overlay.hip", "annot.hip", "crowd.hip", "shade.hip", "track.hip",
               "profile.hip"]
# per-source flags.  chebtile.hip: the gather's fmaf chains must stay scalar v_fma_f32 - SLP-packed v_pk_fma_f32 next to the
# MFMA waves measured 9 % slower over the real-row shapes of a train step (17.2 vs 19.0 ms)
# fscore.hip: the search loop is 6.5 plain f32 instructions per pair (3 v_sub, v_mul, 2 v_fmac, half a v_min3); SLP-packed it
# becomes v_pk_add / v_pk_mul plus v_mov shuffles, which issue at half rate: 1.82 ms against the scalar form's 1.49 ms for
# the launches of an SMPL-size batch of 64
# camfit.hip: include/p2m.h defines the fit's arithmetic as single fp32 operations, each rounded once; contraction to fma would
# change the bits the float64 yardstick (tests/camfit_ref.py) is compared with step by step
# video.hip: the same contract for the One-Euro filter, whose output is pinned bit for bit to the reference's float32 numpy
# arithmetic (tests/video_ref.py)
# crowd.hip: the same contract for the crowd filter's float64 decisions (midpoints, masked means) and the colour formula, which
# are compared exactly with tests/crowd_ref.py
# shade.hip: the same contract for the vertex normals, the barycentric attributes and the smooth shading, which are compared bit
# for bit with tests/shade_ref.py (the flat intensity it shares with render.hip keeps that unit's contraction: p2m_render.h)
# track.hip: the same contract for the tracker's float64 pair costs, which are compared exactly with tests/track_ref.py
# profile.hip: the same contract for the error profile's float64 errors dx dx + dy dy + dz dz, whose bins and sums are compared
# exactly with tests/profile_ref.py
HIP_SOURCE_FLAGS = {"chebtile.hip": ["-fno-slp-vectorize"], "fscore.hip": ["-fno-slp-vectorize"],
                    "camfit.hip": ["-ffp-contract=off"], "video.hip": ["-ffp-contract=off"],
                    "crowd.hip": ["-ffp-contract=off"], "shade.hip": ["-ffp-contract=off"],
                    "track.hip": ["-ffp-contract=off"], "profile.hip": ["-ffp-contract=off"]}
# every header of csrc/ (a source is stale when any of them is newer: none can be forgotten) and the C ABI
HIP_HEADERS = sorted(n for n in os.listdir(CSRC) if n.endswith(".h")) + [os.path.join("..", "..", "include", "p2m.h")]
HIP_LIB = os.path.join(LIBDIR, "libp2m_hip.so")
HOST_LIB = os.path.join(LIBDIR, "libp2m_host.so")


def source_id():
    """Content hash of what the HIP library is built from plus the host-side launch layer (12 hex digits): the identity of
    `the running code` where there is no git (the GPU boxes get a snapshot without .git).  bench.py compares it with the id
    stored in profiles/traffic_latest.json by tools/rocprof_traffic.sh and marks the PMC traffic figures stale when they
    were measured on other code."""
    import hashlib
    h = hashlib.sha1()
    names = [os.path.join(CSRC, n) for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h", ".cpp"))]
    names += [os.path.normpath(os.path.join(CSRC, "..", "..", "include", "p2m.h"))]
    names += [os.path.join(HERE, n) for n in ("ops.py", "meshnet.py", "posenet.py", "cheby_graph_conv.py", "optim.py", "loss.py")]
    for n in names:
        with open(n, "rb") as f:
            h.update(os.path.basename(n).encode() + b"\0" + f.read())
    return h.hexdigest()[:12]


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (set HIPCC)")


def build_hip(force=False, verbose=False):
    """One object per translation unit (compiled in parallel, only the stale ones), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.normpath(os.path.join(CSRC, h)) for h in HIP_HEADERS]
    extra = os.environ.get("P2M_HIPCC_FLAGS", "").split()
    flagfile = os.path.join(objdir, "flags.txt")
    flags_changed = (open(flagfile).read() if os.path.exists(flagfile) else "") != " ".join(extra)
    if not force and not flags_changed and not _stale(HIP_LIB, [os.path.join(CSRC, n) for n in HIP_SOURCES] + hdrs):
        return HIP_LIB                  # (the library is newer than everything it is built from, whatever became of the objects)
    jobs, objs = [], []
    for src_name in HIP_SOURCES:
        src = os.path.join(CSRC, src_name)
        obj = os.path.join(objdir, src_name.replace(".hip", ".o"))
        objs.append(obj)
        if force or flags_changed or _stale(obj, [src] + hdrs):
            jobs.append([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c"]
                        + HIP_SOURCE_FLAGS.get(src_name, []) + extra + ["-o", obj, src])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=CSRC)
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(run, jobs))
        open(flagfile, "w").write(" ".join(extra))
    if jobs or not os.path.exists(HIP_LIB):
        run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", HIP_LIB] + objs)
    return HIP_LIB


def build_host(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    src = os.path.join(CSRC, "p2m_host.cpp")
    if not force and not _stale(HOST_LIB, [src]):
        return HOST_LIB
    cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", HOST_LIB, src]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, cwd=CSRC)
    return HOST_LIB


def build_all(force=False, verbose=False):
    return build_hip(force, verbose), build_host(force, verbose)


if __name__ == "__main__":
    if "--source-id" in sys.argv:
        print(source_id())
    else:
        print(build_all(force="--force" in sys.argv, verbose=True))
