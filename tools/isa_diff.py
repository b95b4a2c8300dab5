#!/usr/bin/env python3
"""Compare two device assembly listings (hipcc -S --cuda-device-only) kernel by kernel.

    python tools/isa_diff.py base.s new.s [--only REGEX] [--max-move PERCENT]

Per kernel symbol of either file one line: `identical` (same body after stripping comments and the function ordinal of the
.LBB<n>_ labels), `missing` (in one file only), or `different` with the instruction count, NumVgprs, ScratchSize and LDSByteSize
of both sides.  A summary follows.  With --max-move the exit status is 1 if a kernel is missing, if NumVgprs, ScratchSize or
LDSByteSize of a kernel differ, or if an instruction count moved by more than PERCENT.  Needs no GPU and no compiler: it reads
only the text and that metadata, and hashes bodies.
"""
import argparse
import hashlib
import re
import sys

META = ("NumVgprs", "ScratchSize", "LDSByteSize")


def kernels(path):
    """{symbol: (body hash, instruction count, {metadata})} of every kernel (a function followed by an .amdhsa_kernel block)."""
    text = open(path).read()
    out = {}
    is_kernel = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\w+)\s*$", text, re.M))
    for m in re.finditer(r"^(\w+):\s*(?:;.*)?\n", text, re.M):
        name = m.group(1)
        end = text.find(".Lfunc_end", m.end())
        if end < 0 or name not in is_kernel:
            continue
        if re.search(r"^\w+:\s*(?:;.*)?\n", text[m.end():end], re.M):     # another global symbol in between: not this function's body
            continue
        lines = []
        for ln in text[m.end():end].splitlines():
            ln = ln.split(";", 1)[0].strip()
            if ln:
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        ninstr = sum(1 for ln in lines if not ln.startswith(".") and not ln.endswith(":"))
        nxt = re.search(r"^\w+:\s*(?:;.*)?\n", text[end:], re.M)      # the metadata comments end before the next symbol
        tail = text[end:end + nxt.start()] if nxt else text[end:]
        meta = {}
        for k in META:
            mm = re.search(r"; %s: (\d+)" % k, tail)
            if not mm:
                sys.exit(f"{path}: kernel {name}: no '; {k}:' line after its body -- is this a -S --cuda-device-only listing?")
            meta[k] = int(mm.group(1))
        out[name] = (hashlib.sha256("\n".join(lines).encode()).hexdigest(), ninstr, meta)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--only", default=None, help="report only kernels whose symbol matches this regex")
    ap.add_argument("--max-move", type=float, default=None, help="fail if an instruction count moves by more than this many percent")
    ap.add_argument("--quiet", action="store_true", help="do not list identical kernels")
    a = ap.parse_args()
    ka, kb = kernels(a.base), kernels(a.new)
    names = sorted(set(ka) | set(kb))
    if a.only:
        names = [n for n in names if re.search(a.only, n)]
    same = diff = missing = bad = 0
    worst = (0.0, None)
    for n in names:
        if n not in ka or n not in kb:
            missing += 1
            print(f"missing    {n} (in {'new' if n not in ka else 'base'} only)")
            continue
        (ha, ia, ma), (hb, ib, mb) = ka[n], kb[n]
        if ha == hb and ma == mb:
            same += 1
            if not a.quiet:
                print(f"identical  {n}")
            continue
        diff += 1
        move = 100.0 * abs(ib - ia) / max(ia, 1)
        if move > worst[0] or worst[1] is None:
            worst = (move, n)
        meta_moved = ma != mb
        bad += meta_moved or (a.max_move is not None and move > a.max_move)
        print(f"different  {n}: instructions {ia} -> {ib} ({move:.3f} %)  " +
              "  ".join(f"{k} {ma[k]} -> {mb[k]}" for k in META) + ("   <-- resources moved" if meta_moved else ""))
    print(f"{len(names)} kernels: {same} identical, {diff} different, {missing} missing" +
          (f"; largest movement {worst[0]:.3f} % ({worst[1]})" if diff else ""))
    if a.max_move is not None and (bad or missing):
        sys.exit(1)


if __name__ == "__main__":
    main()
