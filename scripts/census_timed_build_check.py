"""The diagnostic counters of the instruction census must not change the timed build.  Two checks, neither needs a GPU:
  python scripts/census_timed_build_check.py            the timed pass-B kernel compiled from the tree, against the same tree with every
                                                        `#ifdef RTD_STAGE_CLOCKS` section resolved as undefined and cut out of the text
                                                        beforehand: the instruction streams must be identical
  python scripts/census_timed_build_check.py --rev REV  against the headers of git revision REV (for a change that only adds counters the
                                                        streams must be identical; otherwise the difference in static VALU instructions
                                                        is printed)
Exit status 0: identical."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instruction_census as ic  # noqa: E402

HEADERS = ("rt_device.h", "rt_render_kernel.h", "rt_launch_consts.h", "rt_modes.h", "rt_extend_map.h", "rt_scene.h", "rt_trig.h", "rt_trig_tables.h")


def strip_diag(text):
    """the text with `#ifdef RTD_STAGE_CLOCKS` sections resolved as undefined (their #else part kept)"""
    out, depth, skip = [], [], False
    for ln in text.splitlines(keepends=True):
        t = ln.strip()
        if re.match(r"#\s*if", t):
            mine = bool(re.match(r"#\s*ifdef\s+RTD_STAGE_CLOCKS\b", t))
            depth.append([mine, skip])
            if mine:
                skip = True
                continue
        elif re.match(r"#\s*else", t) and depth and depth[-1][0]:
            skip = depth[-1][1]
            continue
        elif re.match(r"#\s*endif", t) and depth:
            mine, before = depth.pop()
            if mine:
                skip = before
                continue
        if not skip:
            out.append(ln)
    return "".join(out)


def listing(csrc, include, out):
    os.makedirs(out, exist_ok=True)
    stub = os.path.join(csrc, "_census_stub.hip")
    open(stub, "w").write(ic.STUB)
    try:
        s = os.path.join(out, "hot.s")
        subprocess.run(["hipcc", "--offload-arch=gfx950"] + ic.hipflags() + ["--cuda-device-only", "-S", "-o", s, stub], stderr=subprocess.DEVNULL, check=True)
    finally:
        os.remove(stub)
    return [i for i in ic.instructions(s) if i[0] != ".loc"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="census_check_")
    try:
        mine = listing(ic.CSRC, None, os.path.join(tmp, "tree"))
        other_csrc = os.path.join(tmp, "other", "ray-tracing-fsharp_amd", "csrc")
        os.makedirs(other_csrc)
        os.makedirs(os.path.join(tmp, "other", "include"))
        for h in HEADERS + ("../../include/rtfs_amd.h",):
            src = os.path.normpath(os.path.join(ic.CSRC, h))
            rel = os.path.relpath(src, ic.ROOT)
            if a.rev:
                shown = subprocess.run(["git", "-C", ic.ROOT, "show", f"{a.rev}:{rel}"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
                if shown.returncode != 0:
                    continue  # (a header that revision does not have yet)
                text = shown.stdout
            else:
                text = strip_diag(open(src).read())
            open(os.path.normpath(os.path.join(other_csrc, h)), "w").write(text)
        other = listing(other_csrc, None, os.path.join(tmp, "other_out"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    what = f"revision {a.rev}" if a.rev else "the tree without its RTD_STAGE_CLOCKS sections"
    if mine == other:
        print(f"timed kernel: {sum(1 for i in mine if i[0])} instructions, identical to {what}")
        sys.exit(0)
    v = lambda L: sum(1 for i in L if i[0] and i[0].startswith("v_"))
    print(f"timed kernel differs from {what}: {sum(1 for i in mine if i[0])} instructions ({v(mine)} VALU) against {sum(1 for i in other if i[0])} ({v(other)} VALU)")
    sys.exit(1)


if __name__ == "__main__":
    main()
