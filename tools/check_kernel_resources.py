#!/usr/bin/env python3
"""Register / scratch usage of every kernel in lc2is_amd/csrc (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, no GPU needed).
Fails when a kernel of the hot path spills (scratch > 0): launch bounds such as head_ce_grp_kernel<*, 12, 4>'s (512, 2) or the
256-register NT GEMM kernels rely on the allocator staying inside them.  usage: python tools/check_kernel_resources.py [-j N]"""
import concurrent.futures as cf
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lc2is_amd" / "csrc"
HOT = ("gemm_nt_pp_kernel", "gemm_nt_w384_kernel", "gemm_nt_rows_kernel", "gemm_nt_dma_kernel", "gemm_tn_grouped", "attn_fwd_kernel<64", "attn_fwd_kernel<96",
       "attn_bwd_dq2_kernel<64", "attn_bwd_dkdv_kernel<64", "attn_bwd_dq2_kernel<96", "attn_bwd_dkdv_kernel<96",
       "head_ce_grp_kernel", "head_focal_grp_kernel", "head_sigmoid_grp_kernel", "head_finish_kernel", "head_conf_grp_kernel", "head_ce_pw_grp_kernel", "head_kd_grp_kernel", "ln_fwd_kernel", "ln_bwd_kernel", "sgd_kernel",
       "strong_params_kernel", "strong_apply_kernel", "geo_params_kernel", "geo_apply_kernel", "geo_scores_kernel")
# (geo.hip as built today: geo_params_kernel 30 VGPRs, no LDS; geo_apply_kernel<4096> 56 VGPRs, 48 KB of LDS for the staged source box =
# three blocks of 256 lanes per CU, 3 waves per SIMD; geo_scores_kernel 58 VGPRs, no LDS, 8 waves per SIMD; none uses scratch)
# known, accepted (listed so that a NEW spill is a failure): 12 bytes (one 64-bit address + one dword, stored once in front of the row
# loop) in the 128-register LayerNorm backward at C = 768 — HBM-bound at 5.4 TB/s; compiling it for 3 waves per SIMD instead removes the
# spill and measured slower (round 2), and one base pointer per stream instead of fp32 / bf16 pairs made hipcc demote the row arrays to
# the stack (48-144 bytes in every instantiation; tried in round 5).  Every OTHER kernel of the library must report zero scratch.
ACCEPTED = ("ln_bwd_kernel<3>",)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", o) for o in out]


def one(src):
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{CSRC}", f"-I{ROOT / 'include'}",
           "-Wno-unused-function", "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(src),
           "-o", "/dev/null"]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = dict(name=m.group(1), file=src.name)
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def main():
    jobs = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else 4
    srcs = sorted(CSRC.glob("*.hip"))
    with cf.ThreadPoolExecutor(jobs) as ex:
        rows = [r for rs in ex.map(one, srcs) for r in rs]
    names = demangle([r["name"] for r in rows])
    bad = []
    print(f"{'kernel':90s} {'file':24s} {'VGPR':>5s} {'AGPR':>5s} {'occ':>3s} {'scratch':>7s}")
    for r, n in sorted(zip(rows, names), key=lambda t: (t[0]["file"], t[1])):
        n = re.sub(r"\(.*", "", n)
        hot = any(h in n for h in HOT)
        flag = ""
        if r.get("scratch", 0) > 0:
            flag = "  <-- SPILLS" + (" (hot path)" if hot else "")
            if not any(a in n for a in ACCEPTED):   # (round 5: ANY kernel of the library, not only the hot ones)
                bad.append(n)
        print(f"{n[:90]:90s} {r['file']:24s} {r.get('vgpr', 0):5d} {r.get('agpr', 0):5d} {r.get('occ', 0):3d} {r.get('scratch', 0):7d}{flag}")
    if bad:
        print("\nkernels with scratch:", *bad, sep="\n  ")
        sys.exit(1)
    print("\nno kernel of the library uses scratch")


if __name__ == "__main__":
    main()
