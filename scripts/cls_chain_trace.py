"""The cls-row side chain of the ViT blocks against the main stream, from a rocprofv3 --kernel-trace CSV of bench.py:
  * footprint of every main-stream kernel kind (workgroup, arch + accumulation VGPRs, LDS) and what a CU keeps free beside
    ONE resident workgroup of it (512 registers per lane and 8 wave slots per SIMD, 4 SIMDs, 160 KB of LDS per CU) — an upper
    bound: the trace reports no accumulation registers for library kernels (scripts/kernel_descriptor.py reads the truth);
  * in-step average duration of every kernel kind on the main and on the side queue;
  * per cls launch of a block (in launch order): start after the attention's end, open time (start to end), the main-stream
    kernel that was running when it started, and the slack from the end of the block's last cls launch to the start of the
    next attention (negative: the join waited).
Blocks = the intervals between consecutive attention launches in the last `steps` steps of the trace.
usage: python scripts/cls_chain_trace.py <dir with *kernel_trace.csv | csv> [steps=5]"""
import collections, csv, glob, os, statistics, sys

src = sys.argv[1]
f = src if src.endswith(".csv") else max(glob.glob(src + "/**/*kernel_trace.csv", recursive=True), key=os.path.getmtime)
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])


def kind(r) -> str:
    n = r["Kernel_Name"]
    if "Cijk_" in n:       # library GEMM: macro-tile and whether the epilogue adds a bias
        mt = next((t for t in n.split("_") if t.startswith("MT")), "MT?")
        return f"gemm {mt} {'bias' if '_Bias_' in n else 'nobias'} wg{r['Workgroup_Size_X']} grid{r['Grid_Size_X']}"
    n = n.split("(")[0]
    return n[n.find("vpr::") + 5:] if "vpr::" in n else n[-70:]


att = [r for r in rows if "vpr::attention_kernel" in r["Kernel_Name"]]
blocks_per_step = 24
att = att[-(steps * blocks_per_step + 1):]
main_q = att[0]["Queue_Id"]
t0, t1 = att[0]["s"], att[-1]["s"]
win = [r for r in rows if t0 <= r["s"] < t1]
main = [r for r in win if r["Queue_Id"] == main_q]
side_qs = collections.Counter(r["Queue_Id"] for r in win if "skinny_linear_kernel" in r["Kernel_Name"])
side_q = side_qs.most_common(1)[0][0] if side_qs else None
side = [r for r in win if r["Queue_Id"] == side_q] if side_q != main_q else []
print(f"{f}\nwindow: {len(att) - 1} attention intervals, {(t1 - t0) / steps / 1e3:.1f} us per step; main queue {main_q}, cls queue {side_q}"
      f"{' (in-stream: no side chain)' if not side else ''}")

print("\nmain-stream kernel kinds: footprint of one workgroup and what a CU would keep free beside it AS THE TRACE REPORTS IT: the trace's\n"
      "register columns hold the arch registers only (accumulation registers read 0, also where the kernel descriptor allocates\n"
      "them: scripts/kernel_descriptor.py reads the descriptor), so 'free regs' is an upper bound")
foot = {}
for r in main:
    foot.setdefault(kind(r), r)
for k, r in foot.items():
    wg = int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"])
    v, a, lds = int(r["VGPR_Count"]), int(r["Accum_VGPR_Count"]), int(r["LDS_Block_Size"])
    alloc = (v + a + 7) // 8 * 8
    wps = max(1, wg // 64 // 4)                 # waves of the workgroup on each SIMD
    print(f"  {k:66s} wg {wg:4d}  vgpr {v:3d} + agpr {a:3d} (alloc {alloc:3d})  lds {lds:6d}  scratch {r['Scratch_Size']:>3s} | free per SIMD: "
          f"{512 - wps * alloc:3d} regs, {8 - wps} wave slots; free LDS {160 * 1024 - lds:6d}")

for q, name in ((main, "main"), (side, "cls")):
    d = collections.defaultdict(list)
    for r in q:
        d[kind(r)].append((r["e"] - r["s"]) / 1e3)
    print(f"\n{name} queue: in-step duration per kernel kind (us): launches per step, mean, median, total per step")
    for k, v in sorted(d.items(), key=lambda kv: -sum(kv[1])):
        print(f"  {k:66s} {len(v) / steps:6.1f}  {statistics.mean(v):7.1f}  {statistics.median(v):7.1f}  {sum(v) / steps:8.1f}")

if side:
    per = collections.defaultdict(lambda: collections.defaultdict(list))
    under = collections.defaultdict(collections.Counter)
    slack, chain_end, qkv_end = [], [], []
    for a0, a1 in zip(att, att[1:]):
        cl = [r for r in side if a0["s"] <= r["s"] < a1["s"]]
        if len(cl) != 6 or a1["s"] - a0["s"] > 1_000_000:       # the step's last block (and SALAD's tail) is not a block interval
            continue
        mk = [r for r in main if a0["s"] < r["s"] < a1["s"]]
        for i, r in enumerate(cl):
            tag = f"{i} {kind(r)}"
            per[tag]["start"].append((r["s"] - a0["e"]) / 1e3)
            per[tag]["open"].append((r["e"] - r["s"]) / 1e3)
            run = next((kind(m) for m in mk if m["s"] <= r["s"] < m["e"]), "(nothing)")
            under[tag][run.split(" wg")[0][:40]] += 1
        slack.append((a1["s"] - cl[-1]["e"]) / 1e3)
        chain_end.append((cl[-1]["e"] - a0["e"]) / 1e3)
        if mk:
            qkv_end.append((mk[-1]["e"] - a0["e"]) / 1e3)
    print(f"\ncls chain per block ({len(slack)} blocks): start after attention end, open time (mean / median us), main kernel running at its start")
    for tag, d in per.items():
        top = ", ".join(f"{k} x{n}" for k, n in under[tag].most_common(2))
        print(f"  {tag:62s} start {statistics.mean(d['start']):7.1f}  open {statistics.mean(d['open']):6.1f} / {statistics.median(d['open']):6.1f}   [{top}]")
    print(f"  chain open per block (sum of open times): {sum(statistics.mean(d['open']) for d in per.values()):.1f} us")
    print(f"  chain ends {statistics.mean(chain_end):.1f} us after the attention's end, the block's last main kernel {statistics.mean(qkv_end):.1f} us after it")
    print(f"  slack, end of last cls launch -> start of next attention: mean {statistics.mean(slack):.1f}, min {min(slack):.1f} us; "
          f"{sum(s < 0 for s in slack)} of {len(slack)} negative")
