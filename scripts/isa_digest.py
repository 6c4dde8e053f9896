#!/usr/bin/env python3
"""Per-kernel digest of the `.s` listings `make asm` writes: isa_digest.py build/*.s

One line per function symbol (`_Z...:` up to its `.Lfunc_end`), sorted by name: SHA-1 of the
normalised instruction stream, the instruction count, a SHA-1 of the `.amdhsa_kernel` block and
the registers / scratch / LDS / occupancy the compiler reports for it.  Normalised: `;` comments
and blank lines dropped, `.LBB<n>_` -> `.LBB_` (the number of functions ahead of a kernel in its
file does not matter).  Two builds run the same device code iff their outputs are equal (diff).

--rename OLD=NEW (repeatable) substitutes the plain text OLD by NEW in every listing line before
it is parsed.  A kernel's own name appears in its body and in its `.amdhsa_kernel` block, so after
a change of symbol (a dropped template parameter, say) the older build's listing only compares
equal once its symbols are renamed to the new mangled names:
    isa_digest.py --rename ELb0ELi2EEEv=ELb0EEEv --rename ELb1ELi2EEEv=ELb1EEEv old/decoder_fs.s
"""
import argparse
import hashlib
import re

INFO = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
sha = lambda lines: hashlib.sha1("\n".join(lines).encode()).hexdigest()[:16]
rows = {}
ap = argparse.ArgumentParser(usage="isa_digest.py [--rename OLD=NEW]... LISTING.s...")
ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
ap.add_argument("listings", nargs="+")
args = ap.parse_args()
renames = [r.split("=", 1) for r in args.rename]
if any(len(r) != 2 or not r[0] for r in renames):
    ap.error("--rename takes OLD=NEW")
for path in args.listings:
    name, body, hsa, in_hsa = None, [], [], False
    for raw in open(path):
        for old, new in renames:
            raw = raw.replace(old, new)
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
