"""The compiler's view of two builds of the same kernels, side by side: parses the remark streams of
`hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -c FILE.hip` (stderr; works without a GPU) and prints one row
per kernel, parent next to result: VGPRs, AGPRs, SGPRs, scratch bytes per lane, SGPR / VGPR spills, occupancy (waves/SIMD), LDS bytes.
Then the checks a refactor has to pass: same kernel set (minus the names given with --dropped), equal LDS, no new scratch, no
spill count up, no occupancy down; register counts that moved are listed.
usage: python profiles/kernel_resources_cmp.py --parent P.txt [P2.txt ...] --result R.txt [R2.txt ...] [--dropped SUBSTR ...]"""
import argparse
import re
import subprocess

FIELDS = [("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"), ("SGPRs Spill", "sspill"),
          ("VGPRs Spill", "vspill"), ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "LDS")]


def parse(paths):
    out, cur = {}, None
    for p in paths:
        for line in open(p):
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
            if m and cur is not None:
                for key, short in FIELDS:
                    if m.group(1).strip() == key:
                        cur[short] = int(m.group(2))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"^void tavsr::|\(.*$", "", d) for n, d in zip(names, res)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


ap = argparse.ArgumentParser()
ap.add_argument("--parent", nargs="+", required=True)
ap.add_argument("--result", nargs="+", required=True)
ap.add_argument("--dropped", nargs="*", default=[])
args = ap.parse_args()
P, R = parse(args.parent), parse(args.result)
nice = demangle(sorted(set(P) | set(R)))
short = [s for _, s in FIELDS]
print(f"{'kernel (parent | result)':78s} " + " ".join(f"{s:>11s}" for s in short))
problems, moved = [], []
for k in sorted(P, key=lambda n: nice[n]):
    if k not in R:
        dropped = any(s in nice[k] for s in args.dropped)
        print(f"{nice[k]:78s} " + " ".join(f"{P[k][s]:>5d}|    -" for s in short) + ("   dropped" if dropped else "   MISSING"))
        if not dropped:
            problems.append(f"{nice[k]}: missing from the result")
        continue
    p, r = P[k], R[k]
    print(f"{nice[k]:78s} " + " ".join(f"{p[s]:>5d}|{r[s]:<5d}" for s in short))
    if p["LDS"] != r["LDS"]:
        problems.append(f"{nice[k]}: LDS {p['LDS']} -> {r['LDS']}")
    if p["scratch"] == 0 and r["scratch"] != 0:
        problems.append(f"{nice[k]}: scratch 0 -> {r['scratch']}")
    for s in ("sspill", "vspill"):
        if r[s] > p[s]:
            problems.append(f"{nice[k]}: {s} {p[s]} -> {r[s]}")
    if r["occ"] < p["occ"]:
        problems.append(f"{nice[k]}: occupancy {p['occ']} -> {r['occ']}")
    d = [f"{s} {p[s]} -> {r[s]}" for s in ("VGPR", "AGPR", "SGPR", "scratch", "sspill", "vspill", "occ") if p[s] != r[s]]
    if d:
        moved.append(f"{nice[k]}: " + ", ".join(d))
for k in sorted(set(R) - set(P)):
    problems.append(f"{nice[k]}: new in the result")
print(f"\n{len(P)} kernels in the parent, {len(R)} in the result")
print("\nmoved (allowed where occupancy, spills, scratch and LDS hold):" if moved else "\nno register count moved")
for m in moved:
    print("  " + m)
print("\nFAILED:" if problems else "\nall conditions hold")
for m in problems:
    print("  " + m)
