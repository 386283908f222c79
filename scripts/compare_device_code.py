#!/usr/bin/env python
"""Is the device code of two builds the same, function by function?

For a change that only moves source around (or adds instantiations), every device function of the parent's library must come
out of this revision's instruction for instruction.  The gfx950 code objects of both libraries are disassembled
(check_dpp_hazards.disassemble), split into functions by symbol and pooled by name over all code objects, so a kernel may
move from one translation unit to another.  What legitimately differs between two links is set aside: the addresses (the
`// address:` comments; branch operands are relative already), the zero padding between functions, and the pc-relative
offsets of constant tables (the literal of the `s_add_u32` / `s_addc_u32` pair behind an `s_getpc_b64`).

usage: python scripts/compare_device_code.py PARENT.so THIS.so
       -> counts of identical / different / missing / new functions, the names of those not identical;
          exit 1 if any function of PARENT is different or missing
"""
from __future__ import annotations

import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_dpp_hazards import disassemble  # noqa: E402

_SYMBOL = re.compile(r"^[0-9a-fA-F]+ <(.+)>:\s*$")
_GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):(\d+)\]$")


def functions(text: str) -> dict:
    """disassembly of one code object -> {symbol: [normalised instruction lines]}"""
    out, body, pcrel = {}, None, set()
    for ln in text.splitlines():
        m = _SYMBOL.match(ln)
        if m:
            body, pcrel = out.setdefault(m.group(1), []), set()
            continue
        code = " ".join(ln.split("//")[0].split())
        if body is None or not code or code == "..." or code.startswith("Disassembly of section"):
            continue  # ("...": objdump's mark for the zero padding up to the next function's alignment)
        g = _GETPC.match(code)
        if g:
            pcrel = {f"s{g.group(1)}", f"s{g.group(2)}"}
        elif pcrel and code.startswith(("s_add_u32 ", "s_addc_u32 ")):
            ops = [o.strip() for o in code.split(None, 1)[1].split(",")]
            if len(ops) == 3 and ops[0] == ops[1] and ops[0] in pcrel:  # sN += <distance to the table>
                pcrel.discard(ops[0])
                code = f"{code.split()[0]} {ops[0]}, {ops[1]}, <pcrel>"
        body.append(code)
    return out


def pool(texts) -> dict:
    """{symbol: body} over all code objects; a symbol defined in several of them (an inline function, a per-unit static)
    keeps every distinct body, in sorted order"""
    pooled = {}
    for text in texts:
        for name, body in functions(text).items():
            pooled.setdefault(name, set()).add(tuple(body))
    return {name: sorted(bodies) for name, bodies in pooled.items()}


def compare(parent_texts, this_texts):
    """-> (identical, different, missing, new): sorted lists of symbols"""
    a, b = pool(parent_texts), pool(this_texts)
    identical = sorted(n for n in a if n in b and a[n] == b[n])
    different = sorted(n for n in a if n in b and a[n] != b[n])
    return identical, different, sorted(n for n in a if n not in b), sorted(n for n in b if n not in a)


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__)
        return 2
    identical, different, missing, new = compare(disassemble(argv[1]), disassemble(argv[2]))
    print(f"{len(identical) + len(different) + len(missing)} device functions in {argv[1]}: {len(identical)} identical, "
          f"{len(different)} different, {len(missing)} missing; {len(new)} new in {argv[2]}")
    for what, names in (("DIFFERENT", different), ("MISSING", missing), ("new", new)):
        for n in names:
            print(f"  {what}: {n}")
    for key in ("gram_fast_kernel", "gram_long", "pair_bands_kernel", "grad_reduce_kernel"):
        print(f"  identical with '{key}' in the name: {sum(key in n for n in identical)}")
    return 1 if different or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
