#!/usr/bin/env python3
"""Listing table of the plane contractions (csrc/gemm_planes.hip), as profiles/r08_epilogue_asm_table.txt and
r09_copyout_asm_table.txt:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -o gemm_planes.s pose2mesh_release_amd/csrc/gemm_planes.hip
    python tools/epi_listing.py gemm_planes.s [substring of the kernel names ...]

Per kernel: registers, ScratchSize (bytes per lane), waves per SIMD, LDS bytes | between the first and the last global store of
the kernel: 4-byte and 16-byte global stores, 4-byte and 16-byte global loads, full waits (s_waitcnt vmcnt(0)), counted waits
(vmcnt(N > 0)), scratch loads and stores, ds_read_b128 and ds_write_b32."""
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (instruction lines, metadata dict)} of an amdgcn listing."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?^; Occupancy: \d+)", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        code = body.split(".section")[0].split("\n")
        meta = {k: int(v) for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size) (\d+)", body)}
        occ = re.search(r"; Occupancy: (\d+)", body)
        meta["occ"] = int(occ.group(1)) if occ else -1
        nv = re.search(r"; NumVgprs: (\d+)", body)
        na = re.search(r"; NumAgprs: (\d+)", body)
        meta["vgpr"] = int(nv.group(1)) if nv else -1
        meta["agpr"] = int(na.group(1)) if na else 0
        out[name] = (code, meta)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"^void p2m::|\(p2m::GemmArgs\)$|\(p2m::TnArgs\)$", "", s) for s in r[:len(names)]]


def count(code):
    ins = [l.split(";")[0].strip() for l in code]
    st = [i for i, l in enumerate(ins) if l.startswith("global_store")]
    if not st:
        return None
    seg = ins[st[0]:st[-1] + 1]
    n = lambda pat: sum(bool(re.match(pat, l)) for l in seg)
    return dict(st4=n(r"global_store_dword\s"), st16=n(r"global_store_dwordx4\s"), ld4=n(r"global_load_dword\s"),
                ld16=n(r"global_load_dwordx4\s"), vm0=n(r"s_waitcnt.*vmcnt\(0\)"), vmN=n(r"s_waitcnt.*vmcnt\([1-9]"),
                sld=n(r"scratch_load"), sst=n(r"scratch_store"), dsr=n(r"ds_read_b128\s"), dsw=n(r"ds_write_b32\s"))


def main():
    path, pats = sys.argv[1], sys.argv[2:] or ["k_gemm_planes", "k_gemm_rows_k1"]
    ks = kernels(path)
    names = list(ks)
    rows = []
    for name, dem in zip(names, demangle(names)):
        if not any(p in dem for p in pats):
            continue
        code, meta = ks[name]
        c = count(code)
        if c is None:
            continue
        rows.append((dem, meta, c))
    hdr = f"{'kernel':58s} vgpr agpr scratch occ   lds | st4 st16  ld4 ld16 vmcnt0 vmcntN scr_ld scr_st ds_r128 ds_w32"
    print(hdr)
    for dem, m, c in sorted(rows, key=lambda r: r[0]):
        print(f"{dem:58s} {m['vgpr']:4d} {m['agpr']:4d} {m.get('private_segment_fixed_size', 0):7d} {m['occ']:3d} "
              f"{m.get('group_segment_fixed_size', 0):5d} | {c['st4']:3d} {c['st16']:4d} {c['ld4']:4d} {c['ld16']:4d} {c['vm0']:6d} "
              f"{c['vmN']:6d} {c['sld']:6d} {c['sst']:6d} {c['dsr']:7d} {c['dsw']:6d}")


if __name__ == "__main__":
    main()
