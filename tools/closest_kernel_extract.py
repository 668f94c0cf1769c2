"""Per-workload kernel times of a traced closest-point benchmark run.

    rocprofv3 --kernel-trace --stats -d DIR -o closest -- python tools/closest_point_bench.py --scenes soup,terrain,spheres --calls 10 --cpu > LINES
    python tools/closest_kernel_extract.py DIR/closest_results.db LINES OUT.json [--calls 10]

tools/closest_point_bench.py issues, per workload line, 2 warm-up and --calls timed calls of the kernel without counters, then one call
with counters (its own kernel symbol); no workload there walks a tree deeper than 64 levels, so each call is one dispatch. The
dispatches of `closest_kernel<..., false, false>` in the trace, in time order, are therefore cut into groups of 2 + calls, one per
line in order. OUT.json: per workload the bench line's fields, every timed dispatch's kernel ms, and their median."""
import json
import sqlite3
import statistics
import sys


def main(db_path, lines_path, out_path, calls=10):
    db = sqlite3.connect(db_path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = db.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
    lines = [json.loads(l) for l in open(lines_path) if l.startswith("{")]
    work = [l for l in lines if "cpu_threads" not in l]
    symbol = {"soup": "closest_kernel<float, 0, false, false>", "terrain": "closest_kernel<float, 0, false, false>",
              "spheres": "closest_kernel<double, 1, false, false>"}
    out, cursor = [], {}
    for w in work:
        sym = symbol[w["scene"]]
        ms = cursor.setdefault(sym, [(e - s) / 1e6 for n, s, e in rows if sym in n])
        group, cursor[sym] = ms[:2 + calls], ms[2 + calls:]
        assert len(group) == 2 + calls, ("fewer dispatches than the bench lines need", w)
        out.append(dict(w, kernel_ms_each=[round(x, 4) for x in group[2:]], kernel_ms=round(statistics.median(group[2:]), 4)))
    assert all(not left for left in cursor.values()), "more dispatches than the bench lines account for"
    json.dump(out, open(out_path, "w"), indent=1)
    for w in out:
        print(w["scene"], w["queries"], w["n"], w["radius"], "sorted" if w["sorted"] else "as given", "call", w["ms"], "kernel", w["kernel_ms"])


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(*args[:3], calls=int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 10)
