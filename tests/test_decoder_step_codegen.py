"""The split decoder's hand-ordered window steps in the compiler's own assembly of the product
flags (csrc/decoder_fs.hip window_step / window_step_fin, csrc/decoder_common.h "Pair blocks",
DESIGN.md §4 "hand-ordered window steps"), checked on the CPU for all 12 dec_fs_kernel instances.

A 32x32x16 MFMA holds its SIMD's vector issue for 8 of its 32 cycles; what stands between two
MFMAs hides while its issue costs sum to <= 24 cycles and costs its full price past that.  The
cost model is the issue's: 4 cycles an instruction, 4 (N + 1) for `s_nop N`, nothing for
s_waitcnt, s_barrier and labels.  The EXCESS of the tile loop is the sum over its MFMA gaps of
max(0, cost - 24), leaving out the serial regions (a gap of more than 60 instructions: the tile's
point setup, layer 3's serial write at skip 253, the output store).

  * The excess is at most HALF the parent commit's (PARENT_EXCESS: recorded from the parent's
    assembly with excess() below, not from the code under test).  92 % of the parent's excess sat
    in gaps that held epilogue VALU, work that fits the budget (~112 of a step's 192 hideable
    cycles).
  * A pair block is one asm statement with two accumulator-file MFMAs.  Every gap inside a block,
    and from a block's last MFMA to the next block's first, costs <= 24.  Not covered, because one
    of the two MFMAs is compiled code: the gap in front of a window's first block, the barrier row
    (a window's step 15, no unit) with the gaps on both sides of it, and pairs 2-3 of step 14 of
    the FE_FIN0 / FE_FIN1 windows (bare MFMAs, FE_FIN1's partials written between them).
  * Wait states, which the compiler neither pads inside an asm statement nor knows the MFMAs of
    (decoder_common.h lists the table's rows): no MFMA writes an accumulator register in the 12
    issue slots before a block reads it (8-pass XDL write -> VALU read: 11 wait states, plus one);
    nothing but the accumulate chain touches a block MFMA's D in the 12 slots after it; no VALU
    writes a block MFMA's A / B operands in the 2 slots before it.
"""
import re

import pytest

from tests.test_decoder_codegen import (_instructions, _operands, _regs, _slots,  # noqa: F401
                                        _tile_loop, asm)

DTYPES = {"bf16": "IDF16b", "fp16": "IDF16_"}
INSTANCES = [(dt, w, mode) for dt in DTYPES for w in (256, 512) for mode in (0, 1, 2)]
BUDGET = 24
# epilogue windows in the tile loop's CODE, at either width: layers 1 and 7 and the layer(s) around
# the skip connection are unrolled, layers 5-6 (and 2-3 when 512 wide) are one runtime loop each
WINDOWS = 10
SERIAL = 60
# excess(tile loop) on the parent commit (d0f9d42), by the function below
PARENT_EXCESS = {
    ("bf16", 256, 0): 5348, ("bf16", 256, 1): 5352, ("bf16", 256, 2): 5432,
    ("bf16", 512, 0): 6468, ("bf16", 512, 1): 6472, ("bf16", 512, 2): 6400,
    ("fp16", 256, 0): 7144, ("fp16", 256, 1): 7148, ("fp16", 256, 2): 7244,
    ("fp16", 512, 0): 7020, ("fp16", 512, 1): 7024, ("fp16", 512, 2): 7280,
}


def cost(line):
    if line.endswith(":") or line.startswith(("s_waitcnt", "s_barrier")):
        return 0
    m = re.match(r"s_nop\s+(\d+)", line)
    return 4 * (int(m.group(1)) + 1) if m else 4


def gaps(body):
    """[(index of the MFMA that opens it, index of the one that closes it)]"""
    at = [k for k, l in enumerate(body) if l.startswith("v_mfma")]
    return list(zip(at, at[1:]))


def excess(body):
    total = 0
    for a, b in gaps(body):
        if sum(not l.endswith(":") for l in body[a + 1:b]) > SERIAL:
            continue
        total += max(0, sum(cost(l) for l in body[a + 1:b]) - BUDGET)
    return total


def loop_with_blocks(asm_text, dt, w, mode):
    """The tile loop's instructions (labels included) and, per instruction, the number of the
    asm statement it stands in (None: compiled code)."""
    tag = f"{DTYPES[dt]}Li{w}ELi{mode}E"
    ins = _instructions(asm_text, tag)
    name = [n for n in re.findall(r"^(_ZN3ldm\w+dec_fs_kernel\w+):", asm_text, re.M) if tag in n]
    a = asm_text.index(name[0] + ":")
    blk, cur, n = [], None, 0
    for line in asm_text[a:asm_text.index(".Lfunc_end", a)].split("\n"):
        if line.strip().startswith(";;#ASMSTART"):
            cur, n = n, n + 1
        elif line.strip().startswith(";;#ASMEND"):
            cur = None
        t = line.split(";")[0].strip()
        if t and (t.endswith(":") or not t.startswith(".")):
            blk.append(cur)
    assert len(blk) == len(ins)
    h, e = _tile_loop(ins)
    return ins[h:e + 1], blk[h:e + 1]


def pair_blocks(body, blk):
    """asm statement number -> indices of its MFMAs, for the statements with two MFMAs into the
    accumulator file (layer 0's products are single MFMAs into VGPRs)"""
    by = {}
    for k, l in enumerate(body):
        if blk[k] is not None and l.startswith("v_mfma"):
            by.setdefault(blk[k], []).append(k)
    return {b: ks for b, ks in by.items()
            if len(ks) == 2 and all(_operands(body[k])[0].startswith("a") for k in ks)}


def _aregs(op):
    m = re.fullmatch(r"a(\d+)", op)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"a\[(\d+):(\d+)\]", op)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


@pytest.mark.parametrize("dt,w,mode", INSTANCES)
def test_issue_cost_excess_at_most_half_the_parents(asm, dt, w, mode):  # noqa: F811
    body, _ = loop_with_blocks(asm, dt, w, mode)
    x = excess(body)
    print(f"{dt}/{w}/mode {mode}: excess {x} cycles per tile, parent {PARENT_EXCESS[dt, w, mode]}")
    assert 2 * x <= PARENT_EXCESS[dt, w, mode]


@pytest.mark.parametrize("dt,w,mode", INSTANCES)
def test_gaps_of_the_pair_blocks_fit_the_budget(asm, dt, w, mode):  # noqa: F811
    body, blk = loop_with_blocks(asm, dt, w, mode)
    pb = pair_blocks(body, blk)
    # WINDOWS windows of 15 hand-ordered steps of 4 blocks, less the bare pairs of the two FIN
    # windows' step 14
    assert len(pb) == WINDOWS * 60 - 4, len(pb)
    inblock = {k for ks in pb.values() for k in ks}
    checked, over = 0, []
    for a, b in gaps(body):
        if a in inblock and b in inblock:
            checked += 1
            c = sum(cost(l) for l in body[a + 1:b])
            if c > BUDGET:
                over.append((a, c, body[a + 1:b]))
    print(f"{dt}/{w}/mode {mode}: {len(pb)} pair blocks, {checked} gaps checked, "
          f"{len(over)} over {BUDGET}")
    assert checked >= 2 * len(pb) - 3 * WINDOWS
    assert not over, over[:3]


@pytest.mark.parametrize("dt,w,mode", INSTANCES)
def test_pair_blocks_keep_their_wait_states(asm, dt, w, mode):  # noqa: F811
    body, blk = loop_with_blocks(asm, dt, w, mode)
    pb = pair_blocks(body, blk)
    reads = 0
    for ks in pb.values():
        first, last = ks[0], ks[1]
        # the statement's extent
        lo = first
        while lo > 0 and blk[lo - 1] == blk[first]:
            lo -= 1
        hi = last
        while hi + 1 < len(body) and blk[hi + 1] == blk[first]:
            hi += 1
        for k in range(lo, hi + 1):
            if not body[k].startswith("v_accvgpr_read"):
                continue
            reads += 1
            src = _aregs(_operands(body[k])[1])
            assert len(src) == 1, body[k]
            slots, j = 0, k - 1
            while slots < 12 and j >= 0:
                if body[j].startswith("v_mfma"):
                    assert not src & _aregs(_operands(body[j])[0]), (body[j], body[k], slots)
                slots += _slots(body[j])
                j -= 1
        for k in ks:
            d, a, b, c = _operands(body[k])[:4]
            assert d == c, body[k]                       # accumulates in place
            dr = _aregs(d)
            assert len(dr) == 16, body[k]
            ab = _regs(a) | _regs(b)
            assert len(ab) == 8, body[k]
            slots, j = 0, k + 1
            while slots < 12 and j < len(body):
                if not body[j].endswith(":"):
                    ops = _operands(body[j])
                    touched = set().union(*[_aregs(o) for o in ops]) if ops else set()
                    if touched & dr:
                        # only the accumulate chain: an MFMA with the same D and C
                        assert body[j].startswith("v_mfma") and ops[0] == d and ops[3] == d, \
                            (body[k], body[j], slots)
                slots += _slots(body[j])
                j += 1
            slots, j = 0, k - 1
            while slots < 2 and j >= 0:
                ops = _operands(body[j])
                if body[j].startswith("v_") and not body[j].startswith("v_mfma") and ops:
                    assert not _regs(ops[0]) & ab, (body[j], body[k])
                slots += _slots(body[j])
                j -= 1
    assert reads == 128 * WINDOWS                # every window's set, read inside its blocks


@pytest.mark.parametrize("dt,w,mode", INSTANCES)
def test_plain_group_ends_on_its_read_loads_and_loop_test(asm, dt, w, mode):  # noqa: F811
    """The rolled loops of plain 4-step groups (32 MFMAs, no asm statement): between a group's
    last MFMA and its backward branch stand the step's B read, its two weight loads and the
    loop's add and compare -- 5 instructions.  The parent had 9 there, the ring's wrap test
    among them, and the next group's base (v_mov, v_add) at the loop's top, in the same MFMA gap;
    both now stand in the first gap of the group's last step."""
    body, blk = loop_with_blocks(asm, dt, w, mode)
    lab = {l[:-1]: k for k, l in enumerate(body) if l.endswith(":")}
    loops = 0
    for k, l in enumerate(body):
        m = re.match(r"s_cbranch\w*\s+(\S+)", l)
        if not m or not 0 <= lab.get(m.group(1), k) < k:
            continue
        inner = range(lab[m.group(1)], k)
        mf = [j for j in inner if body[j].startswith("v_mfma")]
        if len(mf) != 32 or any(blk[j] is not None for j in inner):
            continue
        loops += 1
        tail = [x for x in body[mf[-1] + 1:k] if not x.endswith(":") and
                not x.startswith("s_waitcnt")]
        assert len(tail) <= 5, tail
        assert sum(x.startswith("ds_read_b128") for x in tail) == 1, tail
        assert sum(x.startswith("buffer_load_dwordx4") for x in tail) == 2, tail
    assert loops >= 6, loops
