"""The time per kernel of the device JPEG decode, from kernel traces: one run per file of

    rocprofv3 --kernel-trace -d DIR/NAME -o NAME -- python scripts/jpeg_measure.py --once FILE      (FILE: a path, or `earth`)

leaves DIR/NAME/NAME_results.db; this script sums every kernel's dispatches in each and divides by the decodes the run made (--once
decodes three times, the first one cold), into the table of profiles/r26/jpeg_kernel_times.json.

usage: python scripts/jpeg_kernel_times.py DIR NAME [NAME ...] [--decodes 3] [--out FILE]"""
import argparse
import json
import os
import sqlite3
import sys


def kernel_times(db_path, decodes):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), sum(end - start) from kernels group by name order by 3 desc").fetchall()  # (ns)
    total = sum(r[2] for r in rows)
    return {"decodes_profiled": decodes, "kernel_us_per_decode": round(total / decodes / 1e3, 1),
            "kernels": [{"kernel": name.split("(")[0], "launches_per_decode": count / decodes, "us_per_decode": round(ns / decodes / 1e3, 1),
                         "share": round(ns / total, 4)} for name, count, ns in rows]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("names", nargs="+")
    ap.add_argument("--decodes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {name: kernel_times(os.path.join(args.dir, name, name + "_results.db"), args.decodes) for name in args.names}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
