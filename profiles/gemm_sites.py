#!/usr/bin/env python3
"""k_gemm_p per launch site from a rocprofv3 --kernel-trace run of the headline bench: the three bottleneck GEMMs share one kernel, so
--stats gives one line for all of them.  gru_fc is told by its grid (N = 2176: more workgroups than the two N = 1536 projections);
gru_ih0 (K = 2176) and gru_ih1 (K = 512) have the same grid and are split at the geometric mean of their shortest and longest launch
(a factor 3 apart, alone and under overlap).  Launches of the warm-up step are left in: they are the same launches.

  python profiles/gemm_sites.py <dir-with-*_kernel_trace.csv> [label]"""
import csv
import glob
import math
import statistics
import sys


def main():
    src = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
    label = sys.argv[2] if len(sys.argv) > 2 else src
    rows = [(int(r["Grid_Size_X"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(open(src)) if "k_gemm_p<" in r["Kernel_Name"]]
    grids = sorted({g for g, _ in rows})
    if len(grids) != 2:
        sys.exit(f"{label}: expected two k_gemm_p grids, found {grids}")
    proj = [d for g, d in rows if g == grids[0]]
    cut = math.sqrt(min(proj) * max(proj))
    sites = {"gru_ih0": [d for d in proj if d >= cut], "gru_ih1": [d for d in proj if d < cut], "gru_fc": [d for g, d in rows if g == grids[1]]}
    for name, d in sites.items():
        d.sort()
        print(f"{label} {name}: {len(d)} launches  mean {statistics.fmean(d) / 1e3:7.2f} us  median {d[len(d) // 2] / 1e3:7.2f}  min {d[0] / 1e3:7.2f}  max {d[-1] / 1e3:7.2f}")


if __name__ == "__main__":
    main()
