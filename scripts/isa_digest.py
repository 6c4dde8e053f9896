#!/usr/bin/env python3
"""Per-kernel digest of the `.s` listings `make asm` writes: isa_digest.py build/*.s

One line per function symbol (`_Z...:` up to its `.Lfunc_end`), sorted by name: SHA-1 of the
normalised instruction stream, the instruction count, a SHA-1 of the `.amdhsa_kernel` block and
the registers / scratch / LDS / occupancy the compiler reports for it.  Normalised: `;` comments
and blank lines dropped, `.LBB<n>_` -> `.LBB_` (the number of functions ahead of a kernel in its
file does not matter).  Two builds run the same device code iff their outputs are equal (diff).
"""
import hashlib
import re
import sys

INFO = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
sha = lambda lines: hashlib.sha1("\n".join(lines).encode()).hexdigest()[:16]
rows = {}
for path in sys.argv[1:]:
    name, body, hsa, in_hsa = None, [], [], False
    for raw in open(path):
        m = re.match(r"; (\w+): *(\d+)", raw)
        if m and m.group(1) in INFO and name in rows:   # the "Kernel info" comments after the end
            rows[name] += f" {m.group(1)}={m.group(2)}"
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", raw.split(";")[0]).strip()
        if not line:
            continue
        m = re.match(r"(_Z\w+):$", line)
        if m:
            name, body, hsa = m.group(1), [], []
        elif line.startswith(".Lfunc_end") and body:
            n = sum(1 for x in body if re.match(r"[a-z]\w* |[a-z]\w*$", x))
            rows[name] = f"{name} isa={sha(body)} n={n} hsa={sha(hsa)}"
            body = []
        elif line.startswith(".amdhsa_kernel") or in_hsa:
            in_hsa = not line.startswith(".end_amdhsa_kernel")
            hsa.append(line)
        elif name:
            body.append(line)
print("\n".join(rows[k] for k in sorted(rows)))
