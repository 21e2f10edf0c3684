"""Per-step medians of the DLRM step's read-after-write chain from a rocprofv3 --kernel-trace CSV
(bench.py --steps 30): the train kernel, the train -> apply hop, the apply walk
(seg_group32_kernel), the fix-up sweep, the fix-up -> next train hop, the sort kernels and the
step span (train start to next train start), over the steps from --skip on; then one step's
timeline like tools/step_timeline.py.
python tools/apply_shape_trace.py TRACE.csv [--skip 8] > out.txt"""
import argparse
import csv
import statistics as st

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--skip", type=int, default=8)
a = ap.parse_args()
rows = sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"]))
S = lambda r: int(r["Start_Timestamp"]) / 1e3
E = lambda r: int(r["End_Timestamp"]) / 1e3
idx = [i for i, r in enumerate(rows) if "dlrm_train_chunk" in r["Kernel_Name"]]
SORT = ("slot_sort_hist0", "slot_sort_scatter0", "slot_sort_hist1", "slot_sort_scatter1")
cols = {k: [] for k in ("train", "train->apply", "apply", "fixup", "fixup->train", "step", *SORT)}
for lo, hi in zip(idx[a.skip:-1], idx[a.skip + 1:]):
    step = rows[lo:hi]
    find = lambda name: next((r for r in step if name in r["Kernel_Name"]), None)
    tr, ap_, fx = rows[lo], find("seg_group32_kernel"), find("seg_fixup_sweep")
    if ap_ is None or fx is None:
        continue
    cols["train"].append(E(tr) - S(tr))
    cols["train->apply"].append(S(ap_) - E(tr))
    cols["apply"].append(E(ap_) - S(ap_))
    cols["fixup"].append(E(fx) - S(fx))
    cols["fixup->train"].append(S(rows[hi]) - E(fx))
    cols["step"].append(S(rows[hi]) - S(tr))
    for k in SORT:
        r = find(k)
        if r is not None:
            cols[k].append(E(r) - S(r))
print(f"# medians over {len(cols['step'])} steps (us): median  [min .. max]")
for k, v in cols.items():
    if v:
        print(f"{k:22s} {st.median(v):8.1f}  [{min(v):7.1f} .. {max(v):7.1f}]")
ap_row = next(r for r in rows[idx[a.skip]:] if "seg_group32_kernel" in r["Kernel_Name"])
print(f"# apply launch: grid {ap_row['Grid_Size_X']} workgroup {ap_row['Workgroup_Size_X']}")
k = min(a.skip + 5, len(idx) - 2)
lo, hi = idx[k], idx[k + 1]
t0 = S(rows[lo])
print(f"# step {k}")
for r in rows[lo:hi]:
    print(f"{S(r) - t0:8.1f} {E(r) - S(r):7.1f} q{r['Queue_Id']} {r['Kernel_Name'][:100]}")
print(f"step span {S(rows[hi]) - t0:.1f}")
