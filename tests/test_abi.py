"""CPU: the C-ABI library builds for gfx950, loads, and exports exactly what include/p2m.h declares."""
import os
import re

import numpy as np

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "p2m.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(p2m_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound(hip_libs):
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/p2m.h but not exported"
        assert n in _lib.HIP_SYMBOLS, f"{n} has no ctypes prototype"
    assert sorted(_lib.HIP_SYMBOLS) == names, "ctypes table and header disagree"
    assert b"gfx950" in lib.p2m_version()
    assert lib.p2m_stats_tile_rows() == 128


def test_host_library_loads(hip_libs):
    from pose2mesh_release_amd import _lib
    assert b"p2m-host" in _lib.host().p2m_host_version()


def test_code_object_is_gfx950(hip_libs):
    so = open(hip_libs[0], "rb").read()
    assert b"gfx950" in so and b"k_gemm_planes" in so and b"k_basis_fwd" in so


def test_every_hip_source_is_built():
    """build.HIP_SOURCES is exactly the *.hip files of csrc/: a source that is not listed is never compiled, and every header of
    csrc/ makes the library stale."""
    from pose2mesh_release_amd import build
    on_disk = {n for n in os.listdir(build.CSRC) if n.endswith(".hip")}
    assert set(build.HIP_SOURCES) == on_disk
    assert len(build.HIP_SOURCES) == len(on_disk), "a source is listed twice"
    assert set(build.HIP_SOURCE_FLAGS) <= on_disk
    assert {n for n in os.listdir(build.CSRC) if n.endswith(".h")} <= set(build.HIP_HEADERS)


def test_product_never_imports_oracle():
    """The product path must not route through oracle/ (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "pose2mesh_release_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "meshnet_oracle" not in txt and "coarsen_oracle" not in txt and "ref_loader" not in txt, f


def test_cpu_tensors_fail_loudly(hip_libs):
    import torch
    from pose2mesh_release_amd import meshnet, synth
    from pose2mesh_release_amd._lib import P2MError
    _, gL, _, J = synth.make_graphs("mano")
    net = meshnet.get_model(5, 3, gL)
    with pytest.raises(P2MError):
        net(torch.zeros(2, J, 5))


def test_class_representatives_cpu_logic():
    from pose2mesh_release_amd import ops as o
    fake = [2, 3, 4, 5, 6, 7, 9, 12, 13, 14, 15]
    rep, m = o.class_representatives(16, fake, 2)
    assert rep.tolist() == [0, 1, 2, 2, 4, 4, 4, 4, 8, 9, 10, 11, 12, 12, 12, 12]
    rep1, _ = o.class_representatives(16, fake, 1)
    assert rep1.tolist() == [0, 1, 2, 2, 4, 4, 6, 6, 8, 9, 10, 11, 12, 12, 14, 14]
    assert o.class_representatives(16, fake, 0)[0].tolist() == list(range(16))


def test_slice_arithmetic_host_logic():
    """Host side of P2M_ARITH_F16X2 (no GPU): headroom of an effective weight, the knob's values, and the scale exponent
    rule of csrc/p2m_split.h restated (U 2^bits 2^s lands in [2^14, 2^15), clamped, 0 for an all-zero tensor)."""
    import subprocess
    import sys
    from pose2mesh_release_amd import ops as o
    assert [o.eff_bits(a, b) for a, b in ((0, 0), (1, 0), (0.5, 0.5), (1, 2), (-0.6, 0.3), (3, 4))] == [0, 1, 1, 2, 1, 3]
    assert {k: v for k, v in zip(("f32", "bf16x3", "f16x2"), (0, 1, 2))} == \
        {a: (setattr(o, "GEMM_ARITH", a), o.arith_code())[1] for a in ("f32", "bf16x3", "f16x2")}
    o.GEMM_ARITH = os.environ.get("P2M_GEMM_ARITH", "f16x2")
    r = subprocess.run([sys.executable, "-c", "import pose2mesh_release_amd.ops"], capture_output=True, text=True,
                       env=dict(os.environ, P2M_GEMM_ARITH="fp8"))
    assert r.returncode != 0 and "P2M_GEMM_ARITH" in r.stderr

    def scale_exp(u, bits):                       # slice_scale_exp(bits of u, bits)
        if u == 0.0:
            return 0
        e = (np.float32(u).view(np.uint32) >> 23) & 0xFF
        return int(np.clip(141 - int(e) - bits, -120, 120))
    for u in (1e-30, 3.7e-7, 0.05, 1.0, 2.0, 7.9, 6.5e4, 1e30):
        for bits in (0, 1, 3):
            s = scale_exp(u, bits)
            if abs(141 - int((np.float32(u).view(np.uint32) >> 23) & 0xFF) - bits) <= 120:
                assert 2.0 ** 14 <= u * 2.0 ** bits * 2.0 ** s < 2.0 ** 15, (u, bits, s)
    assert scale_exp(0.0, 2) == 0 and scale_exp(1e-45, 0) == 120


def test_conv_weights_descriptor_layout():
    """ops._ConvWeightsDesc must be byte-for-byte the p2m_conv_weights of include/p2m.h (72 bytes, natural alignment): the
    descriptor array is built on the host with ctypes and read by the device kernels."""
    import ctypes
    from pose2mesh_release_amd import ops as o
    d = o._ConvWeightsDesc
    assert ctypes.sizeof(d) == 72
    offs = {n: getattr(d, n).offset for n, _ in d._fields_}
    assert offs == {"W": 0, "Fout": 8, "Fin": 12, "fake_a": 16, "fake_b": 20, "eff_bits": 24, "reserved": 28,
                    "Bx_f": 32, "Bx_ef": 40, "Bx_b": 48, "Bx_eb": 56, "amax": 64}
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p2m.h")).read()
    body = hdr[hdr.index("typedef struct p2m_conv_weights {"):hdr.index("} p2m_conv_weights;")]
    order = [m for m in re.findall(r"\b(W|Fout|Fin|fake_a|fake_b|eff_bits|reserved|Bx_f|Bx_ef|Bx_b|Bx_eb|amax)\b", body)]
    assert order == [n for n, _ in d._fields_]


def test_bench_line_helpers_and_cli():
    """bench.py's reporting helpers (no GPU): the per-step statistics, a `dtype` string for every contraction arithmetic that
    spells out the emulation (the line must say what it measured), and the flags the driver's one command relies on."""
    import importlib.util
    import subprocess
    import sys
    spec = importlib.util.spec_from_file_location("p2m_bench", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    st = b.step_stats([10.0, 12.0, 11.0, 13.0, 50.0])
    assert st["median"] == 12.0 and st["min"] == 10.0 and st["max"] == 50.0 and st["p10"] <= st["median"] <= st["p90"]
    assert set(b.DTYPE_NOTE) == {"f16x2", "bf16x3", "f32"}
    assert "2 scaled fp16 slices" in b.DTYPE_NOTE["f16x2"] and "22-bit" in b.DTYPE_NOTE["f16x2"]
    assert "3 exact bf16 slices" in b.DTYPE_NOTE["bf16x3"] and b.DTYPE_NOTE["f32"].startswith("f32 (native")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--also", "--no-arith-ab", "--mode", "--train-graph", "--full",
                 "--dump-outputs"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--also", "nonsense"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "unknown leg" in r.stderr
    # the extra legs belong to --full; a plain run is the headline only
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--also", "infer"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--full" in r.stderr


def test_bench_dump_helpers(tmp_path):
    """bench.py --dump-outputs (no GPU): float32 DIR/<name>.npy per output of the last step, the flat parameter / gradient
    buffers as one fixed seeded sample (ascending, the same indices for both), an array over its cap cut to a fixed seeded
    sample of its leading-axis rows, 64 MB at most in all."""
    import importlib.util
    import types

    import torch
    spec = importlib.util.spec_from_file_location("p2m_bench", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    n = 3_000_000
    opt = types.SimpleNamespace(numel=n, flat_param=torch.arange(n, dtype=torch.float32),
                                flat_grad=-torch.arange(n, dtype=torch.float32))
    mesh = torch.randn(1024, 3000, 3)                         # 36.9 MB: over the mesh cap
    step = types.SimpleNamespace(outputs=(mesh, torch.randn(1024, 17, 3, dtype=torch.float64)),
                                 perm=torch.arange(2999, -1, -1), opt=opt)
    arrays = b.step_outputs(step, torch.tensor(2.5, dtype=torch.float64, requires_grad=True) * 1, False)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), arrays)
    names = ["grads.npy", "lift_pose.npy", "loss.npy", "mesh.npy", "params.npy"]
    assert sorted(os.listdir(tmp_path / "a")) == names
    z = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert all(a.dtype == np.float32 for a in z.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64e6
    assert z["loss"].tolist() == [2.5] and z["lift_pose"].shape == (1024, 17, 3)
    p, g = z["params"], z["grads"]
    assert p.shape == (1 << 20,) and (np.diff(p) > 0).all() and (p == -g).all()
    rows = z["mesh"]
    assert rows.shape[1:] == (3000, 3) and 0 < rows.shape[0] < 1024 and rows.nbytes <= 32 << 20
    full = mesh.flip(1).numpy()                                # the perm gather, reversed order
    hit = [int(np.flatnonzero((full == r).all(axis=(1, 2)))[0]) for r in rows[:8]]
    assert hit == sorted(hit)
    for f in names:                                            # the same sample in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
