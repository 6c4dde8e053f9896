"""The split decoder's epilogue windows in the compiler's own assembly of the product flags
(csrc/decoder_fs.hip, DESIGN.md §4 "epilogue windows"), checked on the CPU for all 12
dec_fs_kernel instances (2 dtypes x 2 widths x 3 modes).

A finished accumulator set is converted between the MFMAs of a later part.  Left to itself the
register allocator copied the whole set into VGPRs at that part's START instead: 83-89
v_accvgpr_read back to back behind the last MFMA of the aux step, with the matrix pipe idle,
7-9 times per tile.  Every such read now sits in an MFMA gap that holds covered work (the
window's own VALU slots, or for layer 1 part 1 the plain steps before the window); the one burst
that remains is layer 3's serial write at skip 253 (a whole set, 128 reads, between two
barriers).  Leading the allocator there must not cost accumulator shuffles, spills or code size,
which is what the other checks hold."""
import re

import pytest

from tests.test_decoder_codegen import _instructions, _tile_loop, asm  # noqa: F401  (asm: fixture)

DTYPES = {"bf16": "IDF16b", "fp16": "IDF16_"}
INSTANCES = [(dt, w, mode) for dt in DTYPES for w in (256, 512) for mode in (0, 1, 2)]
# a legitimate gap holds at most 24 reads (a double epilogue unit), a burst 83 or more
MAX_READS_PER_GAP = 32
# non-label instructions of the tile loop on the parent commit, counted by loop_body() below
PARENT_LOOP_INSTRUCTIONS = {
    ("bf16", 256, 0): 9410, ("bf16", 256, 1): 9365, ("bf16", 256, 2): 9623,
    ("bf16", 512, 0): 9228, ("bf16", 512, 1): 9183, ("bf16", 512, 2): 9425,
    ("fp16", 256, 0): 10771, ("fp16", 256, 1): 10722, ("fp16", 256, 2): 10986,
    ("fp16", 512, 0): 10476, ("fp16", 512, 1): 10427, ("fp16", 512, 2): 10688,
}
# .vgpr_spill_count on the parent commit: none in any instance
PARENT_SPILLS = 0


def loop_body(asm_text, dt, w, mode):
    ins = _instructions(asm_text, f"{DTYPES[dt]}Li{w}ELi{mode}E")
    h, e = _tile_loop(ins)
    return [l for l in ins[h:e + 1] if not l.endswith(":")]


def reads_per_gap(body):
    """v_accvgpr_read counts between consecutive v_mfma"""
    gaps, cur = [], None
    for l in body:
        if l.startswith("v_mfma"):
            if cur is not None:
                gaps.append(cur)
            cur = 0
        elif cur is not None and l.startswith("v_accvgpr_read"):
            cur += 1
    return gaps


@pytest.mark.parametrize("dt,w,mode", INSTANCES)
def test_no_accumulator_burst_with_the_matrix_pipe_idle(asm, dt, w, mode):  # noqa: F811
    gaps = reads_per_gap(loop_body(asm, dt, w, mode))
    assert len(gaps) > 1000, len(gaps)                # the unrolled window and aux steps
    big = [g for g in gaps if g > MAX_READS_PER_GAP]
    print(f"{dt}/{w}/mode {mode}: gaps over {MAX_READS_PER_GAP}: {big}, largest other "
          f"{max(g for g in gaps if g <= MAX_READS_PER_GAP)}")
    if w == 256:
        assert big in ([], [128]), big          # layer 3's serial write, a whole set
    else:
        assert big == [], big


@pytest.mark.parametrize("dt,w,mode", INSTANCES)
def test_no_accumulator_shuffles_or_scratch_in_the_tile_loop(asm, dt, w, mode):  # noqa: F811
    body = loop_body(asm, dt, w, mode)
    bad = [l for l in body if l.startswith(("scratch_", "v_accvgpr_write", "v_accvgpr_mov"))]
    assert not bad, (len(bad), bad[:4])


def test_spill_counts_no_higher_than_the_parents(asm):  # noqa: F811
    found = re.findall(r"\.name:\s+_ZN3ldm\w+dec_fs_kernelIDF16[b_]Li(?:256|512)ELi\dE\w+\n"
                       r"(?:.*\n){0,12}?\s+\.vgpr_spill_count:\s+(\d+)", asm)
    assert len(found) == 12, found
    assert all(int(n) <= PARENT_SPILLS for n in found), found


@pytest.mark.parametrize("dt,w,mode", INSTANCES)
def test_tile_loop_no_longer_than_the_parents(asm, dt, w, mode):  # noqa: F811
    n = len(loop_body(asm, dt, w, mode))
    print(f"{dt}/{w}/mode {mode}: {n} instructions, parent "
          f"{PARENT_LOOP_INSTRUCTIONS[dt, w, mode]}")
    assert n <= PARENT_LOOP_INSTRUCTIONS[dt, w, mode]
