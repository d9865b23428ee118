#!/usr/bin/env python3
"""Per-kernel digest of a built library's gfx950 code: {demangled kernel name: sha1 of its disassembly without addresses}.
Used to check that a refactoring of the host code / a split into translation units left every kernel's instructions as
they were:  tools/kernel_digest.py old.so new.so  -> kernels only in one, kernels whose code differs.
Further arguments PATTERN=REPLACEMENT (a regular expression and its substitution, applied in order) rename the first library's
kernels before the comparison, for a change that renames kernels on purpose.  Each is split at its first '=': PATTERN itself
cannot contain one.
--no-params (anywhere on the command line) compares the kernels by their names without the parameter lists: a parameter whose
type becomes a dependent name (a typedef of a traits template) demangles differently though it is the same type.  Overloads
that differ in their parameters alone then count as one name with several bodies, compared as a multiset.

Example, the change that gave the flooding record kernels a `bool F16` (16-bit flags) -- fourth template argument of
cn_minsum_rec_kernel, last of vn_free_rec_kernel and of vn_kernel (profiles/record_flags.txt has the output):
  tools/kernel_digest.py parent.so new.so --no-params \
      '(cn_minsum_rec_kernel<\w+, \d+, \d+), =\\1, false, ' \
      '(vn_free_rec_kernel<\w+, \d+, \d+)>=\\1, false>' \
      '(vn_kernel<[^>]*)>=\\1, false>'
lists the kernels only in the second library (the F16 = true instantiations) and exits 1 if there are any, or if a body of the
first is missing or differs."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def digests(path):
    data = open(path, "rb").read()
    out, pos = {}, 0
    while True:
        i = data.find(b"\x7fELF", pos)
        if i < 0:
            break
        if struct.unpack_from("<H", data, i + 18)[0] == 224:
            shoff = struct.unpack_from("<Q", data, i + 40)[0]
            shentsize, shnum = struct.unpack_from("<HH", data, i + 58)
            with tempfile.NamedTemporaryFile(suffix=".elf", delete=False) as f:
                f.write(data[i:i + shoff + shentsize * shnum])
            try:
                text = subprocess.run([OBJDUMP, "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", f.name], check=True,
                                      capture_output=True, text=True).stdout
            finally:
                os.unlink(f.name)
            name, body = None, []
            for ln in text.splitlines() + ["<end>:"]:
                m = re.match(r"^(?:[0-9a-f]+ )?<(.*)>:$", ln)
                if m:
                    if name is not None and not name.startswith("L") :
                        # branch targets carry absolute addresses in comments: drop everything after "//"
                        lines = [re.sub(r"\s*//.*", "", b) for b in body]
                        # pc-relative distances to the constant tables (s_getpc_b64, then s_add_u32 sN, sN, <distance>)
                        # depend on where the linker put the kernel: not the kernel's code
                        for k in range(1, len(lines)):
                            if lines[k - 1].startswith("s_getpc_b64") and lines[k].startswith("s_add_u32"):
                                lines[k] = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", lines[k])
                        while lines and lines[-1] in ("", "...", "s_nop 0", "s_code_end"):   # padding behind the kernel's last instruction
                            lines.pop()
                        h = hashlib.sha1("\n".join(lines).encode()).hexdigest()
                        out.setdefault(name, []).append(h)
                    name, body = m.group(1), []
                else:
                    body.append(ln.strip())
        pos = i + 4
    return out


def without_params(name):
    """`void ns::kernel<...>(A, B)` -> `void ns::kernel<...>`"""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += {")": 1, "(": -1}.get(name[i], 0)
        if depth == 0:
            return name[:i]
    return name


if __name__ == "__main__":
    no_params = "--no-params" in sys.argv
    sys.argv = [x for x in sys.argv if x != "--no-params"]
    a, b = digests(sys.argv[1]), digests(sys.argv[2])
    if no_params:
        a, b = ({k2: sum((v for k, v in d.items() if without_params(k) == k2), []) for k2 in {without_params(k) for k in d}}
                for d in (a, b))
    for rename in sys.argv[3:]:
        pattern, replacement = rename.split("=", 1)
        renamed = {}
        for k, v in a.items():
            renamed.setdefault(re.sub(pattern, replacement, k), []).extend(v)
        a = renamed
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    diff = sorted(k for k in set(a) & set(b) if sorted(a[k]) != sorted(b[k]))
    print(f"{sum(len(v) for v in a.values())} kernel bodies in {sys.argv[1]}, {sum(len(v) for v in b.values())} in {sys.argv[2]}")
    print(f"only in the first: {len(only_a)}; only in the second: {len(only_b)}; same name, different code: {len(diff)}")
    for k in (only_a + only_b + diff)[:40]:
        print("  ", k[:200])
    sys.exit(1 if (only_a or only_b or diff) else 0)
