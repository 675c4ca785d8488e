"""csrc/rt_job_plan.h alone (tests/c/job_plan_table.cpp): the present set of a render job -- the prefix of units of the fused kernel or
pass A, less the live list's entries pass B did not reach -- against a small Python model of the prefix rule, over unit sizes 1, 16 and
64, pixel counts that are and are not multiples of the unit, interleaved shards, done_a in {0, 1, middle, last, total, beyond}, done_b in
{0, 1, middle, n_list, beyond} and an empty live list, each prefix reached once by the counter and once by the budget.  Three deliberate
faults in a copy of the header must each fail the comparison.  Built plainly, and once as a stand-alone program under
-fsanitize=address,undefined."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc", "rt_job_plan.h")
TABLE = os.path.join(ROOT, "tests", "c", "job_plan_table.cpp")


def model(passes, chunk, cols, row_first, row_stride, n_rows, queue_a, queue_b, limit_a, limit_b, live):
    """The prefix rule, restated: a pixel is present iff its unit is below done_a and (two passes) it is not a live-list entry at an
    index >= done_b; the counters clamped to their totals and to the budget."""
    n = n_rows * cols
    units = -(-n // chunk)
    done_a = min(queue_a, units) if limit_a < 0 else min(queue_a, units, limit_a)
    done_b = 0
    present = [lp // chunk < done_a for lp in range(n)]
    if passes == 2:
        done_b = min(queue_b, len(live)) if limit_b < 0 else min(queue_b, len(live), limit_b)
        for i, lp in enumerate(live):
            if i >= done_b:
                present[lp] = False
    glob = [(row_first + (lp // cols) * row_stride) * cols + lp % cols for lp in range(n) if present[lp]]
    return f"{units} {done_a} {done_b} {sum(present)} | " + "".join("1" if p else "0" for p in present) + " |" + "".join(f" {g}" for g in glob)


def cases():
    rnd = random.Random(28)
    out = []
    shards = [(7, 0, 1, 5), (13, 1, 2, 5), (16, 0, 1, 4), (64, 2, 3, 3), (71, 0, 1, 41), (9, 0, 1, 0)]  # (cols, row_first, row_stride, n_rows)
    for chunk in (1, 16, 64):
        for cols, row_first, row_stride, n_rows in shards:
            n = n_rows * cols
            units = -(-n // chunk)
            for done_a in sorted({0, 1, units // 2, max(units - 1, 0), units, units + 5}):
                for reach in ("counter", "budget"):
                    qa, la = (done_a, -1) if reach == "counter" else (units + 9, done_a)
                    out.append((1, chunk, cols, row_first, row_stride, n_rows, qa, 0, la, -1, []))
                    # two passes: the list holds pixels of the rendered units only (pass A made it), in an order of its own
                    rendered = [lp for lp in range(n) if lp // chunk < min(done_a, units)]
                    for live in ([], rnd.sample(rendered, len(rendered) // 2), rnd.sample(rendered, len(rendered))):
                        m = len(live)
                        for done_b in sorted({0, 1, m // 2, m, m + 3}):
                            qb, lb = (done_b, -1) if reach == "counter" else (m + 7, done_b)
                            out.append((2, chunk, cols, row_first, row_stride, n_rows, qa, qb, la, lb, live))
    return out


CASES = cases()
CLIP = "clip 4 2 0 0 0 3 4 2 0 2 1 0"  # rtjob::clip_reservation over the table's fixed (first, want, total, limit)


def build(tmp_path, header=HEADER, flags=()):
    tree = tmp_path / "tree"
    os.makedirs(tree / "tests" / "c")
    os.makedirs(tree / "ray-tracing-fsharp_amd" / "csrc")
    shutil.copy(TABLE, tree / "tests" / "c" / "job_plan_table.cpp")
    shutil.copy(header, tree / "ray-tracing-fsharp_amd" / "csrc" / "rt_job_plan.h")
    exe = str(tmp_path / "job_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", *flags, "-o", exe, str(tree / "tests" / "c" / "job_plan_table.cpp")])
    return exe


def run(exe):
    text = "".join(" ".join(str(v) for v in c[:10]) + f" {len(c[10])} " + " ".join(str(e) for e in c[10]) + "\n" for c in CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


def mismatches(lines):
    assert len(lines) == 1 + len(CASES)
    return (lines[0] != CLIP) + sum(got.rstrip() != model(*c).rstrip() for got, c in zip(lines[1:], CASES))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_header_gives_the_models_present_set(tmp_path, sanitize):
    assert len(CASES) > 1500
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    assert mismatches(run(build(tmp_path, flags=flags))) == 0


FAULTS = {
    "the clamp to the total dropped": ("uint64_t d = counter < total ? counter : total;", "uint64_t d = counter;"),
    ">= done_b made > done_b": ("return index >= done_b; }", "return index > done_b; }"),
    "the pass-A prefix ignored under two passes": ("present[lp] = unit_done(pl, lp, done_a) ? 1u : 0u;",
                                                   "present[lp] = (pl.passes == 2 || unit_done(pl, lp, done_a)) ? 1u : 0u;"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_deliberate_fault_fails_the_comparison(tmp_path, fault):
    old, new = FAULTS[fault]
    text = open(HEADER).read()
    assert text.count(old) == 1, "the header no longer has the line this fault edits"
    broken = tmp_path / "rt_job_plan.h"
    broken.write_text(text.replace(old, new))
    assert mismatches(run(build(tmp_path, header=str(broken)))) > 0
