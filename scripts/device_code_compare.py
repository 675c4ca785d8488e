"""Compares two `make asm` outputs (csrc directories holding rtfs_amd.gfx950.s and resource_usage.txt): per family of kernels, how many of the
parent's functions have an identical instruction stream here (labels normalised, .amdhsa_kernarg_size left out) and identical resource
figures; functions that differ only in hexadecimal constants and offsets (the arguments behind a RenderParams that grew) are named as such.
  python scripts/device_code_compare.py PARENT_CSRC BRANCH_CSRC            -> profiles/rNN/device_code_vs_parent.txt
  python scripts/device_code_compare.py PARENT_CSRC BRANCH_CSRC --views    -> ... then the views kernels beside their twins (resources_views.txt)
  python scripts/device_code_compare.py PARENT_CSRC BRANCH_CSRC --camera-hits-views -> ... then the camera-hits-views kernels beside their twins
  python scripts/device_code_compare.py PARENT_CSRC BRANCH_CSRC SYMBOL     -> ... then a diff of one function"""
import re, sys, collections
def funcs(path):
    out = {}
    name = None; body = []
    for line in open(path):
        m = re.match(r'^(_Z\w+|\w+):\s*(;.*)?$', line)
        if name is None:
            if m and not line.startswith('.'):
                name = m.group(1); body = []
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = body; name = None; continue
        l = line.split(';')[0].rstrip()
        if not l.strip() or '.amdhsa_kernarg_size' in l: continue
        l = re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', l)
        l = re.sub(r'\.Ltmp\d+', '.Ltmp', l)
        body.append(l)
    return out
def resources(path):
    out = {}; cur = None
    for line in open(path):
        m = re.search(r'remark: .*Function Name: (\S+)', line)
        if m: cur = m.group(1); out[cur] = []; continue
        m = re.search(r'remark:\s+(.*\S)\s*\[-Rpass', line)
        if m and cur: out[cur].append(m.group(1))
    return out
short = lambda n: re.sub(r'^_ZN12_GLOBAL__N_1\d+', '', n).split('EN3rtd')[0]
pa, br = sys.argv[1], sys.argv[2]
fa, fb = funcs(pa + '/rtfs_amd.gfx950.s'), funcs(br + '/rtfs_amd.gfx950.s')
ra, rb = resources(pa + '/resource_usage.txt'), resources(br + '/resource_usage.txt')
fam = lambda n: (re.match(r'_ZN3rtd\d+(\w+?kernel)I', n) or re.match(r'()', n)).group(1) or 'other functions'
groups = collections.defaultdict(list)
for n in fa: groups[fam(n)].append(n)
for g, names in sorted(groups.items(), key=lambda kv: -len(kv[1])):
    missing = [n for n in names if n not in fb]
    same = [n for n in names if n in fb and fa[n] == fb[n]]
    kern = [n for n in names if n in ra]  # (kernels: device functions that are not kernels have no resource remark)
    sres = [n for n in kern if n in rb and ra[n] == rb[n]]
    line = f"{g}: {len(names)} in the parent; {len(missing)} missing here; {len(same)} with an identical instruction stream (labels normalised); {len(sres)} of {len(kern)} kernels with identical resource figures"
    ch = [n for n in names if n in fb and fa[n] != fb[n]]
    if ch:
        import difflib
        only_offsets = [n for n in ch if len(fa[n]) == len(fb[n]) and all(re.sub(r'offset:\d+|0x[0-9a-f]+\b', 'K', x) == re.sub(r'offset:\d+|0x[0-9a-f]+\b', 'K', y) for x, y in zip(fa[n], fb[n]))]
        line += f"; differing only in kernel-argument offsets (their arguments follow RenderParams, which grew by 40 bytes): " + (str(sorted(short(n) for n in only_offsets)) if g == 'other functions' else f"all {len(only_offsets)}")
        rest = [n for n in ch if n not in only_offsets]
        if rest: line += f"; OTHERWISE CHANGED: {rest[:12]}"
    print(line)
new = collections.Counter(fam(n) for n in fb if n not in fa)
for g, c in new.items(): print(f"{g}: {c} (new)")
if len(sys.argv) > 3 and sys.argv[3] == '--views':
    print()
    print("# Resource figures of the views kernels beside their twins (make asm, -Rpass-analysis=kernel-resource-usage)")
    print("# render_views_kernel<LDS, COUNT, BLOCK, PASS, TEX> vs render_kernel<LDS, COUNT, BLOCK, PASS, TEX>")
    def fig(r):
        d = dict(x.split(': ') for x in r if ': ' in x)
        return f"VGPRs {d['VGPRs']}, SGPRs {d['TotalSGPRs']}, scratch {d['ScratchSize [bytes/lane]']} B/lane, VGPR spills {d['VGPRs Spill']}, SGPR spills {d['SGPRs Spill']}, occupancy {d['Occupancy [waves/SIMD]']}"
    worse = []
    for n in sorted(rb):
        m = re.match(r'_ZN3rtd19render_views_kernelILb(\d)ELb(\d)ELi(\d+)ELi(\d)ELb(\d)EEE', n)
        if not m: continue
        twin = n.replace('19render_views_kernel', '13render_kernel')
        print(f"lds={m.group(1)} count={m.group(2)} block={m.group(3)} pass={m.group(4)} tex={m.group(5)}")
        print("   views: " + fig(rb[n])); print("   twin:  " + fig(rb[twin]))
        dv, dt = (dict(x.split(': ') for x in r if ': ' in x) for r in (rb[n], rb[twin]))
        if int(dv['VGPRs Spill']) > 0 and int(dt['VGPRs Spill']) == 0: worse.append(n)
    print(f"# views kernels that spill VGPRs where the twin does not: {len(worse)} {worse}")
elif len(sys.argv) > 3 and sys.argv[3] == '--camera-hits-views':
    print()
    print("# Resource figures of the camera-hits-views kernels beside their twins (make asm, -Rpass-analysis=kernel-resource-usage)")
    print("# camera_hits_views_kernel<LDS, COUNT, BLOCK> vs render_kernel<LDS, COUNT, BLOCK, 14, false>")
    def fig(r):
        d = dict(x.split(': ') for x in r if ': ' in x)
        return f"VGPRs {d['VGPRs']}, SGPRs {d['TotalSGPRs']}, scratch {d['ScratchSize [bytes/lane]']} B/lane, VGPR spills {d['VGPRs Spill']}, SGPR spills {d['SGPRs Spill']}, occupancy {d['Occupancy [waves/SIMD]']}"
    worse, seen = [], 0
    for n in sorted(rb):
        m = re.match(r'_ZN3rtd\d+camera_hits_views_kernelILb(\d)ELb(\d)ELi(\d+)EEE', n)
        if not m: continue
        seen += 1
        twin = [t for t in rb if re.match(rf'_ZN3rtd13render_kernelILb{m.group(1)}ELb{m.group(2)}ELi{m.group(3)}ELi14ELb0EEE', t)][0]
        print(f"lds={m.group(1)} count={m.group(2)} block={m.group(3)}")
        print("   views: " + fig(rb[n])); print("   twin:  " + fig(rb[twin]))
        dv, dt = (dict(x.split(': ') for x in r if ': ' in x) for r in (rb[n], rb[twin]))
        if (int(dv['VGPRs Spill']) > 0 and int(dt['VGPRs Spill']) == 0) or (int(dv['ScratchSize [bytes/lane]']) > 0 and int(dt['ScratchSize [bytes/lane]']) == 0): worse.append(n)
    print(f"# kernels listed: {seen}; that use scratch or spill VGPRs where the twin does not: {len(worse)} {worse}")
elif len(sys.argv) > 3:
    import difflib
    n = sys.argv[3]
    d = list(difflib.unified_diff(fa[n], fb[n], lineterm='', n=1))
    print(len(fa[n]), len(fb[n]), len(d)); print("\n".join(d[:60]))
