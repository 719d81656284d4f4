"""python tools/experiments/session_trace_compare.py DIR_PARENT DIR_NEW MARKS OUT.md [NPZ_PARENT NPZ_NEW] — per handle and hardware queue,
ordered (kernel, grid, workgroup) lists; with the two sessions' result files, also which of their arrays differ bytewise."""
import csv, glob, gzip, os, sqlite3, sys


def load(d):
    rows = []  # (start, queue, name, grid, wg)
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    csvs = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if csvs:
        for r in csv.DictReader(open(csvs[0])):
            rows.append((int(r["Dispatch_Id"]), r["Queue_Id"], r["Kernel_Name"],
                         (r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]), (r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])))
    elif dbs:
        cur = sqlite3.connect(dbs[0]).cursor()
        cur.execute("select * from kernels")
        cols = [c[0] for c in cur.description]
        print("db columns:", cols)
        ix = lambda pred: [i for i, c in enumerate(cols) if pred(c.lower())]
        name, start = cols.index("name"), cols.index("start")
        q = ix(lambda c: "queue" in c)[:1]
        g = ix(lambda c: "grid" in c)
        w = ix(lambda c: "workgroup" in c)
        assert q and g and w, cols
        for r in cur:
            rows.append((int(r[start]), str(r[q[0]]), r[name], tuple(str(r[i]) for i in g), tuple(str(r[i]) for i in w)))
    else:
        raise SystemExit(f"no trace under {d}")
    rows.sort()
    with gzip.open(os.path.join(d, "extracted.txt.gz"), "wt") as f:
        for r in rows:
            f.write(f"{r[1]}|{r[2]}|{','.join(r[3])}|{','.join(r[4])}\n")
    return rows


def windows(rows, n_marks):
    """split at the op-tier gelu launches (the marker between handles)"""
    cuts = [r[0] for r in rows if "gelu" in r[2].lower() and "gemv" not in r[2].lower() and "prefill" not in r[2].lower() and "gemm" not in r[2].lower()]
    print("markers:", len(cuts), "expected", n_marks + 1)
    out, cur, k = [], [], 0
    for r in rows:
        if k < len(cuts) and r[0] == cuts[k]:
            out.append(cur)
            cur = []
            k += 1
            continue
        cur.append(r)
    out.append(cur)
    return out


def per_queue(rows):
    qs = {}
    for r in rows:
        if "__amd_rocclr_copyBuffer" in r[2]:
            continue
        qs.setdefault(r[1], []).append((r[2], r[3], r[4]))
    return list(qs.values())  # queues in order of first use


def main():
    dp, dn, marks, out = sys.argv[1:5]
    names = ["(init)"] + open(marks).read().split("\n")[:-1] + ["(tail)"]
    a, b = load(dp), load(dn)
    print("dispatches:", len(a), len(b))
    wa, wb = windows(a, len(names) - 2), windows(b, len(names) - 2)
    lines = ["| handle | launches, parent | launches, this change | ordered lists |", "|---|---|---|---|"]
    bad = 0
    for i in range(max(len(wa), len(wb))):
        qa, qb = per_queue(wa[i]) if i < len(wa) else [], per_queue(wb[i]) if i < len(wb) else []
        same = qa == qb
        if not same:
            bad += 1
            for x, y in zip(qa, qb):
                for j, (u, v) in enumerate(zip(x, y)):
                    if u != v:
                        print("first difference in", names[i] if i < len(names) else i, "at", j)
                        for t in range(max(0, j - 3), min(len(x), len(y), j + 4)):
                            print("   ", t, x[t][0][:70], x[t][1], "|", y[t][0][:70], y[t][1])
                        break
        nm = names[i] if i < len(names) else f"#{i}"
        if not qa and not qb:
            continue
        lines.append(f"| {nm} | {' + '.join(str(len(x)) for x in qa)} | {' + '.join(str(len(x)) for x in qb)} | {'identical' if same else 'DIFFERENT'} |")
    lines.append("")
    lines.append(f"{len(a)} / {len(b)} dispatches per trace (copy kernels included); {bad} handles differ")
    if len(sys.argv) > 6:
        import numpy as np

        za, zb = np.load(sys.argv[5]), np.load(sys.argv[6])
        diff = [k for k in sorted(set(za.files) | set(zb.files))
                if k not in za.files or k not in zb.files or za[k].dtype != zb[k].dtype or za[k].shape != zb[k].shape or za[k].tobytes() != zb[k].tobytes()]
        lines.append(f"{len(za.files)} / {len(zb.files)} result arrays; {len(diff)} differ bytewise" + (": " + ", ".join(diff[:20]) if diff else ""))
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


main()
