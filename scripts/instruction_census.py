"""Instruction census of the timed pass-B kernel, render_kernel<true,false,1024,2,false>: where a frame's VALU wave-instructions
are issued.  Static side: the kernel alone, compiled with line tables, split into basic blocks with VALU counts by class.
Dynamic side: executions per block group from the stage statistics of a -DRTD_STAGE_CLOCKS build (scripts/one_frame.py
--census-dump).  The table is static x executions, cost-weighted with the issue costs measured in profiles/r3/valu_rates.txt
and reconciled with the SQ_INSTS_VALU* counters of a one-frame PMC run (scripts/pmc.sh).

  python scripts/instruction_census.py compile [--out DIR] [-D MACRO ...]   stub + listings; checks that line tables change no instruction
  python scripts/instruction_census.py blocks LISTING                       the static table, one row per basic block
  python scripts/instruction_census.py table LISTING STATS.json [PMC.csv]   the census (profiles/r5/instruction_census.txt)
Needs no GPU."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc")
KERNEL = "_ZN3rtd13render_kernelILb1ELb0ELi1024ELi2ELb0EEEvNS_12RenderParamsE"
STUB = """#include "../../include/rtfs_amd.h"
#include "rt_device.h"
#include "rt_render_kernel.h"
template __global__ void rtd::render_kernel<true, false, 1024, 2, false>(const rtd::RenderParams);
"""
CLASSES = ("f64_add", "f64_mul", "f64_fma", "f64_other", "f64_trans", "f32", "int", "cmp", "selmov", "cvt", "xlane")
# issue cost in cycles per wave64 instruction at 4 waves per SIMD (profiles/r3/valu_rates.txt, last row): the class's measured member,
# or the mean of its measured members
COST = {"f64_add": 5.30, "f64_mul": 5.46, "f64_fma": 5.83, "f64_other": 5.5, "f64_trans": 17.1, "f32": 3.9, "int": 4.2, "cmp": 5.5,
        "selmov": 4.1, "cvt": 4.8, "xlane": 4.2}
COST_OP = {"v_cndmask_b32": 4.96, "v_mov_b32": 3.22, "v_add_u32": 3.70, "v_xor_b32": 3.46, "v_lshlrev_b32": 4.92, "v_mul_lo_u32": 4.86,
           "v_alignbit_b32": 5.43, "v_fma_f32": 3.44, "v_add_f32": 3.40, "v_max_f32": 4.87, "v_max3_f32": 5.21, "v_min3_f32": 5.64,
           "v_ldexp_f64": 5.06, "v_div_scale_f64": 5.90, "v_div_fixup_f64": 5.60, "v_rndne_f64": 4.92, "v_max_f64": 5.32,
           "v_cvt_f64_u32": 4.71, "v_cvt_f32_f64": 4.96, "v_rcp_f64": 17.22, "v_rsq_f64": 16.96}


def classify(op):
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    if re.match(r"v_(readlane|writelane|readfirstlane|mbcnt|permlane|mov_b32_dpp|bpermute)", base) or op.endswith("_dpp"):
        return "xlane"
    if base.startswith(("v_cmp", "v_cmpx")):
        return "cmp"
    if base.startswith("v_cvt"):
        return "cvt"
    if base in ("v_cndmask_b32", "v_mov_b32", "v_mov_b64", "v_accvgpr_read_b32", "v_accvgpr_write_b32", "v_swap_b32"):
        return "selmov"
    if base.endswith("_f64"):
        if base in ("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64"):
            return "f64_trans"
        if base == "v_add_f64":
            return "f64_add"
        if base == "v_mul_f64":
            return "f64_mul"
        if base in ("v_fma_f64", "v_fmac_f64", "v_div_fmas_f64"):
            return "f64_fma"
        return "f64_other"
    if re.search(r"_f(32|16)$", base):
        return "f32"
    return "int"


def cost_of(op):
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    return COST_OP.get(base, COST[classify(op)])


def hipflags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()


def instructions(path, sym=KERNEL):
    """[(op, rest)] of one function of a listing, labels as (None, label)"""
    out, on = [], False
    for ln in open(path):
        if ln.startswith(sym + ":"):
            on = True
            continue
        if not on:
            continue
        if ln.startswith(".Lfunc_end"):
            break
        m = re.match(r"(\.LBB\d+_\d+|\d+):", ln)  # (numeric ones: the local labels of inline assembly, the hand-written node loop)
        if m:
            out.append((None, m.group(1)))
            continue
        m = re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", ln)
        if m:
            out.append((".loc", (int(m.group(1)), int(m.group(2)))))
            continue
        if re.match(r"\s*; rare arm\b", ln):  # RTD_RARE_ARM (rt_device.h): the head of an arm behind a wave-uniform guard
            out.append((".rare", None))
            continue
        m = re.match(r"\s+((?:v|s|ds|global|scratch|buffer|flat)_\w+)\s*(.*?)\s*(;.*)?$", ln)
        if m:
            out.append((m.group(1), m.group(2)))
    return out


def file_table(path):
    files = {}
    for ln in open(path):
        m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', ln)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
    return files


_src = {}


def func_of(f, l):
    if f not in ("rt_device.h", "rt_render_kernel.h"):
        return f
    if f not in _src:
        _src[f] = open(os.path.join(CSRC, f)).read().splitlines()
    L = _src[f]
    for i in range(min(l, len(L)) - 1, -1, -1):
        m = re.match(r"^\s{0,4}(?:template.*>\s*)?(?:RTD_INLINE|__device__|__global__|__host__)[^;]*?(\w+)\(", L[i])
        if m:
            return m.group(1)
    return "?"


class Block:
    def __init__(self, idx, label):
        self.idx, self.label = idx, label
        self.ops = []  # (op, (file, line))
        self.succ = []  # labels
        self.falls = True
        self.names = []
        self.rare = False  # part of an arm behind a wave-uniform guard (RTD_ANY_LANE): not on the common path

    def valu(self):
        return [o for o in self.ops if o[0].startswith("v_")]

    def by_class(self):
        c = collections.Counter()
        for op, _ in self.valu():
            c[classify(op)] += 1
        return c

    def cost(self):
        return sum(cost_of(op) for op, _ in self.valu())

    def where(self):
        """the (function, file, line) most of the block's VALU instructions were written on; of all its instructions if it has none"""
        ops = self.valu() or self.ops
        fn = collections.Counter((func_of(*loc), loc[0]) for _, loc in ops if loc)
        if not fn:
            return ("?", "?", 0)
        (f, fl), _ = fn.most_common(1)[0]
        ln = collections.Counter(loc[1] for _, loc in ops if loc and loc[0] == fl and func_of(*loc) == f).most_common(1)[0][0]
        return (f, fl, ln)


def blocks(path):
    """basic blocks in layout order: a block starts at a label and after every branch"""
    files = file_table(path)
    out, cur, loc = [], Block(0, "entry"), None
    for op, rest in instructions(path):
        if op is None:
            if cur.ops:
                out.append(cur)
                cur = Block(len(out), rest)
            elif cur.label is None or cur.label == "entry":
                cur.label = rest
            cur.names.append(rest)
            continue
        if op == ".rare":
            cur.rare = True
            continue
        if op == ".loc":
            if rest[1] != 0 or loc is None:  # (line 0: compiler-made code, counted with the line before it)
                loc = (files.get(rest[0], str(rest[0])), rest[1])
            continue
        cur.ops.append((op, loc))
        if op.startswith(("s_cbranch", "s_branch")) or op in ("s_endpgm", "s_setpc_b64"):
            if op.startswith(("s_cbranch", "s_branch")):
                cur.succ.append(rest.split()[0])
            cur.falls = op.startswith("s_cbranch")
            out.append(cur)
            cur = Block(len(out), None)
    if cur.ops:
        out.append(cur)
    # a guarded arm: the block behind the guard's scalar branch carries the marker; the arm is that block and what it falls or
    # branches into without a label of its own (the join, and every loop header, has one)
    for i, b in enumerate(out):
        if b.rare and not (i and out[i - 1].rare):
            for nb in out[i + 1:]:
                if nb.names:
                    break
                nb.rare = True
    return out


def loop_depth(bl):
    """layout-order loop nesting: the number of backward branches (target at or before the branch) that span the block"""
    at = {}
    for b in bl:
        for n in b.names:
            at[n] = b.idx
    depth = [0] * len(bl)
    spans = set()
    for b in bl:
        for s in b.succ:
            if re.fullmatch(r"\d+b", s):  # a numeric local label, backwards: the nearest one before the branch
                prev = [x.idx for x in bl[:b.idx + 1] if s[:-1] in x.names]
                if prev:
                    spans.add((prev[-1], b.idx))
            elif s in at and at[s] <= b.idx:
                spans.add((at[s], b.idx))
    for lo, hi in spans:
        for i in range(lo, hi + 1):
            depth[i] += 1
    return depth, spans


def cmd_compile(a):
    out = os.path.abspath(a.out)
    os.makedirs(out, exist_ok=True)
    stub = os.path.join(CSRC, "_census_stub.hip")  # beside the headers, as rtfs_amd.hip is: the same include paths
    open(stub, "w").write(STUB)
    try:
        base = ["hipcc", "--offload-arch=gfx950"] + hipflags() + ["-D" + d for d in a.D] + ["--cuda-device-only", "-S"]
        plain, lined = os.path.join(out, "hot.s"), os.path.join(out, "hot_lines.s")
        res = subprocess.run(base + ["-o", plain, stub, "-Rpass-analysis=kernel-resource-usage"], stderr=subprocess.PIPE, text=True, check=True)
        open(os.path.join(out, "hot_resources.txt"), "w").write(res.stderr)
        subprocess.run(base + ["-gline-tables-only", "-o", lined, stub], stderr=subprocess.DEVNULL, check=True)
    finally:
        os.remove(stub)
    p, l = [i for i in instructions(plain) if i[0] != ".loc"], [i for i in instructions(lined) if i[0] != ".loc"]
    if p != l:
        sys.exit(f"-gline-tables-only changed the code: {len(p)} against {len(l)} instructions and labels")
    print(f"{lined}: {sum(1 for i in p if i[0])} instructions, equal to the build without line tables")


def fmt_classes(c):
    return " ".join(f"{c.get(k, 0):4d}" for k in CLASSES)


def cmd_blocks(a):
    bl = blocks(a.listing)
    depth, _ = loop_depth(bl)
    print(f"# {a.listing}: {len(bl)} basic blocks, {sum(len(b.valu()) for b in bl)} VALU instructions")
    print("# blk depth label        VALU " + " ".join(f"{k[-4:]:>4}" for k in CLASSES) + "  cost  SALU LDS VMEM  written in")
    for b in bl:
        f, fl, ln = b.where()
        n = collections.Counter("s" if op.startswith("s_") else "d" if op.startswith("ds_") else "v" if op.startswith("v_") else "m" for op, _ in b.ops)
        f = f + " [rare arm]" if b.rare else f
        print(f"{b.idx:5d} {depth[b.idx]:3d}   {(b.label or ''):12s} {n['v']:4d} {fmt_classes(b.by_class())} {b.cost():6.0f} {n['s']:4d} {n['d']:3d} {n['m']:3d}   {f} ({fl}:{ln})")


# ---- the table: block groups and their execution counts -------------------------------------------------------------------------
# A block belongs to the stage of the nearest block before it (layout order follows the source) whose code was written in one of the
# stage's marker functions; inside a stage, blocks written in the functions below form groups with execution counts of their own.
STAGE_MARKERS = [  # (function the block was mostly written in, stage)
    ("stage_scene", "prologue"), ("render_kernel", "prologue"), ("make_view", "prologue"), ("Sched", "prologue"),
    ("pixel_candidates", "range"), ("pixel_key", "range"),
    ("unpark_plan", "refill"), ("unpark_lane", "refill"),
    ("stage_slow", "slow"), ("stage_lamb", "lamb"), ("stage_walk", "walk"), ("stage_shade", "shade"), ("wave_sum_u64", "epilogue"), ("amd_warp_functions.h", "epilogue"),
]
GROUPS = [  # (stage or None, function, group name, execution-count key)
    (None, "node_loop_lds32", "walk: node loop (hand-written)", "loop_trips"),
    (None, "pk", "walk: node loop (hand-written)", "loop_trips"),
    ("walk", "leaf_test_object_exact:sliver", "walk: leaf sliver (exact box test)", "sliver_blocks"),
    ("walk", "leaf_test_object_exact", "walk: leaf pass", "leaf_passes"),
    ("walk", "pend_pop", "walk: leaf pass", "leaf_passes"),
    ("walk", "walk_ctx32", "walk: stage entry", "walk_entries"),
    ("walk", "filter_axis", "walk: stage entry", "walk_entries"),
    ("refill", "park_load", "refill: unpark general (global pool)", "unpark_general_batches"),
    ("refill", "park_load_lds", "refill: unpark Lambert (LDS pool)", "unpark_lambert_batches"),
    (None, "start_item", "refill: new items", "new_refills"),
    (None, "camera_ray", "refill: new items", "new_refills"),
    (None, "stream_for", "refill: new items", "new_refills"),
    (None, "mix64", "refill: new items", "new_refills"),
    (None, "mod_m31", "refill: new items", "new_refills"),
    (None, "div_uniform", "refill: new items", "new_refills"),
    ("shade", "unbounded_tests", "shade: unbounded tests, per object", "shade_stages_x_unbounded"),
    ("shade", "sphere_first_intersection", "shade: unbounded sphere test", "shade_stages_x_unbounded_spheres"),
    ("shade", "plane_intersection", "shade: unbounded plane test", "shade_stages_x_unbounded_planes"),
    ("shade", "park_store", "shade: park store general", "store_blocks_general"),
    ("shade", "park_store_lds", "shade: park store Lambert", "store_blocks_lambert"),
    ("shade", "lambert_bounce", "shade: Lambert in place (pool off)", "zero"),
    ("shade", "random_unit", "shade: Lambert in place (pool off)", "zero"),
    ("shade", "rng_next", "shade: Lambert in place (pool off)", "zero"),
    ("shade", "rng_get", "shade: Lambert in place (pool off)", "zero"),
    ("shade", "pix_darken", "shade: Lambert in place (pool off)", "zero"),
    ("shade", "reflection_fast", "shade: light source", "light_batches"),
    ("shade", "pix_combine", "shade: light source", "light_batches"),
]
STAGE_DEFAULT = {"prologue": ("prologue", "waves"), "epilogue": ("epilogue", "waves"), "range": ("range reserve / flush", "ranges"),
                 "refill": ("refill: common", "refill_stages"), "slow": ("slow: general reflection", "slow_stages"),
                 "lamb": ("lamb: Lambert batch", "lamb_batches"), "walk": ("walk: stage entry", "walk_entries"),
                 "shade": ("shade: common", "shade_stages"), "loop": ("loop bookkeeping", "turns")}


def counts_from(stats, unbounded):
    c, ss = dict(stats["census"]), stats["stage_stats"]
    n = max(1, stats.get("launches", 1))
    out = {k: v / n for k, v in c.items() if not isinstance(v, list)}
    out["zero"] = 0
    out.setdefault("guarded_arms", 0)  # (executions per frame: census words 48-50 of a diagnostic build, a few thousand lanes)
    out["waves"] = ss["waves"]
    out.setdefault("loop_trips", ss["wave_ticks"] / n)  # (a diagnostic timed launch keeps the node loop's trips there)
    out["shade_stages_x_unbounded_spheres"] = out.get("shade_stages", 0) * unbounded[0]
    out["shade_stages_x_unbounded_planes"] = out.get("shade_stages", 0) * unbounded[1]
    out["shade_stages_x_unbounded"] = out.get("shade_stages", 0) * sum(unbounded)
    return out


def assign(bl):
    """(group name, count key) per block"""
    out, stage, after_loop = [], "prologue", False
    funcs = [b.where()[0] for b in bl]
    for b in bl:
        f, fl, ln = b.where()
        for fn, st in STAGE_MARKERS:
            if f == fn and stage != "epilogue":
                if st != stage:
                    after_loop = False
                stage = st
        if f in ("run_stream", "pixel_setup", "footprint_setup", "lds_take", "lds_add", "add_result") and stage not in ("prologue", "refill", "epilogue"):
            stage = "loop"  # (run_stream's own lines inside the refill are the item arithmetic: they stay with the refill;
                            #  pixel_setup's and footprint_setup's lines were run_stream's until they became functions, and are counted as they were)
        if f in ("node_loop_lds32", "pk"):
            after_loop = True
        hit = None
        if b.rare:
            out.append(("guarded arms (Equal, +inf): rare", "guarded_arms", stage))
            continue
        for st, fn, name, key in GROUPS:
            if fn.endswith(":sliver"):
                if stage == st and f in ("leaf_test_object_exact", "bbox_hits_nf") and any(classify(o) == "f64_other" and o.startswith("v_div") for o, _ in b.valu()):
                    hit = (name, key)
                    break
                continue
            if (st is None or st == stage) and f == fn:
                hit = (name, key)
                break
        if stage == "shade" and f in ("dot", "vsub") and "plane_intersection" in funcs[b.idx + 1:b.idx + 2]:
            hit = ("shade: unbounded plane test", "shade_stages_x_unbounded_planes")  # the plane's own dot products, laid out before the rest of its test
        if stage == "walk" and after_loop and (hit is None or hit[1] == "walk_entries"):
            hit = ("walk: leaf pass", "leaf_passes")  # everything of the walk stage behind the node loop runs once per leaf pass
        if hit is None:
            # code of helper functions (dot, walk, unitise, math) inherits the group of the block before it inside the same stage
            prev = next((x for x in reversed(out) if x[1] != "guarded_arms"), None)  # (an arm does not hand its group on)
            if prev and prev[2] == stage and f not in [m[0] for m in STAGE_MARKERS] and f not in ("run_stream", "pixel_setup", "footprint_setup"):
                hit = prev[:2]
            else:
                hit = STAGE_DEFAULT[stage]
        out.append((hit[0], hit[1], stage))
    return out


def cmd_table(a):
    bl = blocks(a.listing)
    stats = json.load(open(a.stats))
    cnt = counts_from(stats, (a.unbounded_spheres, a.unbounded_planes))
    groups = collections.OrderedDict()
    for b, (name, key, _) in zip(bl, assign(bl)):
        g = groups.setdefault(name, {"key": key, "static": collections.Counter(), "cost": 0.0, "blocks": 0})
        g["static"].update(b.by_class())
        g["cost"] += b.cost()
        g["blocks"] += 1
    pmc = {}
    if a.pmc and os.path.isdir(a.pmc):  # scripts/pmc.sh's output directory: the rows of this kernel alone
        import csv
        import glob
        for f in glob.glob(os.path.join(a.pmc, "*", "*counter_collection.csv")):
            for r in csv.DictReader(open(f)):
                if re.search(r"render_kernel<true, false, 1024, 2, false>", r["Kernel_Name"]):
                    pmc[r["Counter_Name"]] = pmc.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    elif a.pmc:  # a summary.csv: pass A's and pass B's launches together
        for ln in open(a.pmc):
            if "," in ln and not ln.startswith("#"):
                k, v = ln.strip().split(",")[:2]
                pmc[k] = float(v)
    tot_dyn = sum(sum(g["static"].values()) * cnt.get(g["key"], 0) for g in groups.values())
    tot_cost = sum(g["cost"] * cnt.get(g["key"], 0) for g in groups.values())
    print(f"# instruction census of {KERNEL}")
    print(f"# listing {os.path.basename(a.listing)}: {len(bl)} basic blocks, {sum(len(b.valu()) for b in bl)} static VALU instructions; execution counts: {os.path.basename(a.stats)} (pass B's timed launch of one frame)")
    print("# group: static VALU by class x executions = dynamic wave-instructions; share of the census total; cost-weighted share (profiles/r3/valu_rates.txt, 4 waves per SIMD)")
    print(f"# {'group':42s} {'executions':>13s} {'count key':>26s} {'static':>6s} " + " ".join(f"{k[-5:]:>5s}" for k in CLASSES) + f" {'dynamic':>10s} {'share':>6s} {'cost sh.':>8s}")
    dyn_class = collections.Counter()
    for name, g in sorted(groups.items(), key=lambda kv: -sum(kv[1]["static"].values()) * cnt.get(kv[1]["key"], 0)):
        n = cnt.get(g["key"], 0)
        st = sum(g["static"].values())
        for k, v in g["static"].items():
            dyn_class[k] += v * n
        print(f"  {name:42s} {n:13.4g} {g['key']:>26s} {st:6d} {fmt_classes(g['static']).replace('   ', '  ')} {st * n:10.4g} {100 * st * n / tot_dyn:5.1f}% {100 * g['cost'] * n / tot_cost:7.1f}%")
    print(f"# census total {tot_dyn:.4g} VALU wave-instructions, {tot_cost:.4g} issue cycles")
    lanes = {"lamb: Lambert batch": ("lamb_lanes", "lamb_batches"), "walk: leaf pass": ("leaf_lanes", "leaf_passes"), "refill: new items": ("new_items", "new_refills"),
             "shade: light source": ("light_lanes", "light_batches"), "shade: park store Lambert": ("store_lanes_lambert", "store_blocks_lambert"),
             "shade: common": ("shade_lanes", "shade_stages"), "slow: general reflection": ("slow_lanes", "slow_stages"), "walk: node loop (hand-written)": ("loop_lanes", "loop_trips")}
    print("# lanes active per execution: " + ", ".join(f"{g} {cnt[a_] / cnt[b_]:.1f}" for g, (a_, b_) in lanes.items() if cnt.get(a_) and cnt.get(b_)))
    print("# rare events: " + ", ".join(f"{k} {cnt.get(k, 0):.0f}" for k in ("random_unit_retries", "lambert_bounce_retries", "sliver_lanes", "sliver_blocks")))
    c = stats["census"]
    if "slow_lanes_by_style" in c:
        print(f"# general reflection by style (lanes / stages that held the style, of {c.get('slow_stages', 0)} stages): "
              + ", ".join(f"style {i}: {l} / {b_}" for i, (l, b_) in enumerate(zip(c["slow_lanes_by_style"], c["slow_batches_by_style"])) if l))
    if pmc:
        def line(what, mine, theirs):
            print(f"#   {what:34s} census {mine:12.4g}   counter {theirs:12.4g}   residual {100 * (mine - theirs) / theirs:+6.1f} %")
        other = a.other_valu
        print(f"# reconciliation with {os.path.basename(os.path.normpath(a.pmc))} (" + ("this kernel's launches of one frame" if os.path.isdir(a.pmc) else
              "the frame's render_kernel launches: pass A + pass B; pass A's share is not in the census" + (f", taken as {other:.3g} from --other-valu" if other else "")) + ")")
        line("SQ_INSTS_VALU", tot_dyn + other, pmc.get("SQ_INSTS_VALU", float("nan")))
        f64 = dyn_class["f64_add"] + dyn_class["f64_mul"] + dyn_class["f64_fma"] + dyn_class["f64_trans"]
        line("F64 add+mul+fma+trans", f64, sum(pmc.get("SQ_INSTS_VALU_" + k, 0) for k in ("ADD_F64", "MUL_F64", "FMA_F64", "TRANS_F64")))
        for k, c in (("f64_add", "ADD_F64"), ("f64_mul", "MUL_F64"), ("f64_fma", "FMA_F64"), ("f64_trans", "TRANS_F64")):
            line("  " + c, dyn_class[k], pmc.get("SQ_INSTS_VALU_" + c, float("nan")))
        line("INT32 (class int)", dyn_class["int"], pmc.get("SQ_INSTS_VALU_INT32", float("nan")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compile")
    c.add_argument("--out", default=os.path.join(ROOT, "build_ab", "census"))
    c.add_argument("-D", action="append", default=[])
    c.set_defaults(fn=cmd_compile)
    c = sub.add_parser("blocks")
    c.add_argument("listing")
    c.set_defaults(fn=cmd_blocks)
    c = sub.add_parser("table")
    c.add_argument("listing")
    c.add_argument("stats")
    c.add_argument("pmc", nargs="?")
    c.add_argument("--other-valu", type=float, default=0.0, help="SQ_INSTS_VALU of the frame's other launches (pass A), to set the census beside the frame's counter")
    c.add_argument("--unbounded-spheres", type=int, default=2, help="unbounded objects of the scene by kind (the bench scene: the ground and the dome, both spheres)")
    c.add_argument("--unbounded-planes", type=int, default=0)
    c.set_defaults(fn=cmd_table)
    a = ap.parse_args()
    a.fn(a)
