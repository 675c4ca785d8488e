"""One line per render_kernel instantiation from csrc/resource_usage.txt (`make -C ray-tracing-fsharp_amd/csrc asm`).
With a second argument: one line per kernel whose mangled name contains it (e.g. `of_image_kernel`), LDS and occupancy included."""
import os
import re
import sys

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "ray-tracing-fsharp_amd", "csrc", "resource_usage.txt")
which = sys.argv[2] if len(sys.argv) > 2 else "render_kernel"
txt = open(path).read()
for b in re.split(r"remark: Function Name: ", txt)[1:]:
    name = b.split()[0]
    if which not in name:
        continue
    g = lambda k: re.search(k + r": (\d+)", b).group(1)
    scratch = g(r"ScratchSize \[bytes/lane\]")
    if which != "render_kernel":
        lds, occupancy = g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")
        print(f"{name}  SGPR {g('TotalSGPRs'):>3} VGPR {g('VGPRs'):>3} scratch {scratch:>4} B  SGPR-spill {g('SGPRs Spill'):>3}  VGPR-spill {g('VGPRs Spill'):>3}  "
              f"LDS {lds:>6} B  occupancy {occupancy} waves/SIMD")
        continue
    m = re.search(r"render_kernelILb(\d)ELb(\d)ELi(\d+)ELi(\d+)ELb(\d)", name)
    print(f"LDS={m.group(1)} COUNT={m.group(2)} BLOCK={m.group(3):>4} MODE={m.group(4):>2} TEX={m.group(5)}  SGPR {g('TotalSGPRs'):>3} VGPR {g('VGPRs'):>3} "
          f"scratch {scratch:>4} B  SGPR-spill {g('SGPRs Spill'):>3}  VGPR-spill {g('VGPRs Spill'):>3}")
