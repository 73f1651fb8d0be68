#!/usr/bin/env python3
"""Summary of scripts/prof_sort.sh's two passes: per (kernel, grid size) the mean duration per launch from the kernel trace and the mean
of every counter from the counters-only pass, with the figures derived from them for the sort kernels:
  valu_per_wave        SQ_INSTS_VALU / SQ_WAVES
  busy_per_valu        SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU        (cycles the vector pipe is held per instruction; 4 = full rate)
  valu_busy_per_simd   SQ_ACTIVE_INST_VALU / SIMDs the launch occupies (blocks x 4 when every block has a CU to itself, else 1024)
  kernel_cycles        GRBM_GUI_ACTIVE
usage: collect_sort_prof.py <dir> [kernel substring ...]"""
import collections, csv, glob, os, sys

out = sys.argv[1]
pats = sys.argv[2:] or ["qsort_", "nn_grid_coop"]
clean = lambda n: n.replace("(anonymous namespace)::", "").split("(")[0]
for f in glob.glob(os.path.join(out, "trace", "*", "*_kernel_trace.csv")):
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        n = clean(r["Kernel_Name"])
        if any(p in n for p in pats):
            g = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
            agg[(n, g)].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (n, g), v in sorted(agg.items()):
        print(f"trace {n} grid {g} calls {len(v)} avg_us {sum(v) / len(v) / 1e3:.2f} min {min(v) / 1e3:.2f} max {max(v) / 1e3:.2f}")
for f in glob.glob(os.path.join(out, "pmc", "*", "*_counter_collection.csv")):
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    wg = {}
    for r in csv.DictReader(open(f)):
        n = clean(r["Kernel_Name"])
        if any(p in n for p in pats):
            agg[(n, int(r["Grid_Size"]))][r["Counter_Name"]].append(float(r["Counter_Value"]))
            wg[(n, int(r["Grid_Size"]))] = int(r.get("Workgroup_Size") or 1024)
    for (n, g), c in sorted(agg.items()):
        m = {k: sum(v) / len(v) for k, v in c.items()}
        launches = max(len(v) for v in c.values())
        print(f"pmc {n} grid {g} launches {launches} " + " ".join(f"{k} {v:.0f}" for k, v in sorted(m.items())))
        if all(k in m for k in ("SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "GRBM_GUI_ACTIVE")) and m["SQ_WAVES"]:
            blocks = g // wg[(n, g)]
            simds = min(1024, blocks * max(1, min(4, wg[(n, g)] // 64)))
            print(f"    valu_per_wave {m['SQ_INSTS_VALU'] / m['SQ_WAVES']:.1f} busy_per_valu {m['SQ_ACTIVE_INST_VALU'] / max(m['SQ_INSTS_VALU'], 1):.2f} "
                  f"valu_busy_per_simd {m['SQ_ACTIVE_INST_VALU'] / simds:.0f} (simds {simds}) kernel_cycles {m['GRBM_GUI_ACTIVE']:.0f} "
                  f"valu_busy_share {m['SQ_ACTIVE_INST_VALU'] / simds / max(m['GRBM_GUI_ACTIVE'], 1):.3f} "
                  f"wave_cycles_per_wave {m['SQ_WAVE_CYCLES'] / m['SQ_WAVES']:.0f} wait_any_share {m['SQ_WAIT_ANY'] / max(m['SQ_WAVE_CYCLES'], 1):.3f}")
