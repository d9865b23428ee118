#!/usr/bin/env python3
"""Register / LDS / scratch use of the kernels in the built product library, read from the gfx950 code objects'
metadata notes (no GPU needed).  usage: tools/kernel_resources.py [substring of the demangled kernel name ...]
       tools/kernel_resources.py --gate [library]: the resource gate of the row-shape check-node kernels, for the build"""
import re
import struct
import subprocess
import sys
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ldpc_toolbox_amd", "lib", "libldpc_toolbox.so")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FILT = "/usr/bin/c++filt"


def images(path):
    data = open(path, "rb").read()
    pos = 0
    while True:
        i = data.find(b"\x7fELF", pos)
        if i < 0:
            return
        if struct.unpack_from("<H", data, i + 18)[0] == 224:  # EM_AMDGPU
            shoff = struct.unpack_from("<Q", data, i + 40)[0]
            shentsize, shnum = struct.unpack_from("<HH", data, i + 58)
            yield data[i:i + shoff + shentsize * shnum]
        pos = i + 4


def kernels(lib=None):
    """-> [(demangled name, vgpr, agpr, sgpr, spilled vgprs, scratch bytes, static lds bytes, max workgroup size)]"""
    lib = lib or os.environ.get("LDPC_LIB", LIB)
    rows = []
    for k, img in enumerate(images(lib)):
        tmp = f"/tmp/_kres_{os.getpid()}_{k}.elf"
        open(tmp, "wb").write(img)
        notes = subprocess.run([READELF, "--notes", tmp], capture_output=True, text=True).stdout
        os.unlink(tmp)
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            blk = ".agpr_count:" + blk
            get = lambda key: (re.search(r"\." + key + r":\s+(\S+)", blk) or [None, "?"])[1]
            rows.append((get("name"), get("vgpr_count"), get("agpr_count"), get("sgpr_count"), get("vgpr_spill_count"),
                         get("private_segment_fixed_size"), get("group_segment_fixed_size"), get("max_flat_workgroup_size")))
    names = subprocess.run([FILT], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    return [(nm,) + tuple(int(x) if x.isdigit() else -1 for x in r[1:]) for r, nm in zip(rows, names)]


# cn_minsum_rec_kernel's row-shape form (its twelfth template argument, SHAPE, is 1 or 2): five waves per SIMD is what the
# form was built for, and it has them only because of how its row step is laid out for the compiler (kernels_flooding.hip.h).
# A compiler that lays it out otherwise gives 120 VGPRs or scratch and a slower kernel with the same results: no test sees it.
SHAPE_FORM = re.compile(r"cn_minsum_rec_kernel<(?:[^,<>]+, ){11}[12][,>]")
GATE_VGPRS, GATE_LDS = 96, 16384


def gate(lib):
    """The resource gate of the row-shape kernels -> process exit status (the build's last step)."""
    rows = [k for k in kernels(lib) if SHAPE_FORM.search(k[0])]
    bad = [k for k in rows if not (0 <= k[1] <= GATE_VGPRS and k[2] == 0 and k[4] == 0 and k[5] == 0 and 0 <= k[6] <= GATE_LDS)]
    for k in bad:
        print(f"kernel_resources: over the gate ({GATE_VGPRS} VGPRs, no scratch, {GATE_LDS} B of LDS): vgpr {k[1]} agpr {k[2]} "
              f"spill {k[4]} scratch {k[5]} lds {k[6]}  {k[0][:150]}", file=sys.stderr)
    if not rows:
        print("kernel_resources: no row-shape instantiation of cn_minsum_rec_kernel found: the gate looked at nothing", file=sys.stderr)
    print(f"kernel_resources: {len(rows)} row-shape kernels, {len(bad)} over the gate; most VGPRs {max([k[1] for k in rows] or [0])}")
    return 1 if bad or not rows else 0


def main():
    if "--gate" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--gate"]
        sys.exit(gate(rest[0] if rest else None))
    want = sys.argv[1:]
    rows = [(None,) + tuple(str(x) for x in k[1:]) + (k[0],) for k in kernels()]
    names = [r[-1] for r in rows]
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'spill':>5} {'scratch':>7} {'lds':>6} {'wgmax':>5}  kernel")
    for r, nm in zip(rows, names):
        if want and not all(w in nm for w in want):
            continue
        print(f"{r[1]:>5} {r[2]:>5} {r[3]:>5} {r[4]:>5} {r[5]:>7} {r[6]:>6} {r[7]:>5}  {nm[:150]}")


if __name__ == "__main__":
    main()
