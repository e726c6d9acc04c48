"""The byte masks of the layer step expanded in pairs (sw_mask7x2 / sw_zero_mask2), on the headline instance
lnsfaid_decode4s_kernel<2>: every layer really issues v_lshlrev_b64 - 24 of them, one per pair - and that many fewer 32-bit left
shifts twice over, no register copies pay for the pairs, and the iteration is shorter by what the pairs save.  Counted between the
kernel's own comment lines, on the way an iteration after the first takes, exactly as tests/test_static_layers_isa.py counts (its
walk and tools/isa_layer_trip.py's classes are used).  Cross-compiles the file to gfx950 assembly.  No GPU needed."""
import pytest

from test_static_layers_isa import HEADLINE, _layers, asm, tool  # noqa: F401  (asm, tool: fixtures)

# the parent of this change, commit 642d173, taken once with the same walk from its build
PARENT_SHL32 = [63, 61, 63, 63, 63, 63, 63, 63, 63, 63, 63, 62]  # v_lshlrev_b32 per layer
PARENT_MOVES = 45          # v_mov_b32 on the walk; the whole text between the comment lines holds as many
PARENT_ACCVGPR = 0
PARENT_ITERATION = 10938   # issued instructions of every kind per layered iteration
PAIRS = 24                 # per layer: 11 in pass 1, 11 in pass 2, (nm3, nm4), the two zero masks
# what this tree reaches
SHL64 = [24] * 12
SHL32 = [15, 13, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14]
ITERATION = 10640
WAIT_STATES = 12  # s_nop in front of a reader that follows its 64-bit shift too closely


@pytest.fixture(scope="module")
def walk(asm, tool):
    per = _layers(tool.kernel_body(asm, HEADLINE))
    assert sorted(per) == list(range(12))
    return [per[br] for br in range(12)]


def _count(walk, prefix):
    return [sum(1 for i in ins if i.startswith(prefix)) for ins in walk]


def test_every_layer_shifts_in_pairs(walk):
    b64, b32 = _count(walk, "v_lshlrev_b64"), _count(walk, "v_lshlrev_b32")
    print("v_lshlrev_b64 per layer %s, v_lshlrev_b32 per layer %s (parent %s)" % (b64, b32, PARENT_SHL32))
    assert all(n >= 1 for n in b64), b64
    assert all(new <= old - 22 for new, old in zip(b32, PARENT_SHL32)), b32
    assert all(n <= want for n, want in zip(b64, SHL64)) and all(n <= want for n, want in zip(b32, SHL32)), (b64, b32)
    # two shifts became one: a pair that cost a third instruction would show here
    assert all(old - new == 2 * pairs for new, old, pairs in zip(b32, PARENT_SHL32, b64)), (b32, b64)


def test_no_copies_pay_for_the_pairs(walk, asm, tool):
    moves, acc = sum(_count(walk, "v_mov_b32")), sum(_count(walk, "v_accvgpr_"))
    body = tool.kernel_body(asm, HEADLINE)
    hot = [l.split(";")[0].strip() for l in body[body.index("; lf4s layers begin"):body.index("; lf4s layers end")].split("\n")]
    text_moves = sum(1 for i in hot if i.startswith(("v_mov_b32", "v_mov_b64")))
    text_acc = sum(1 for i in hot if i.startswith("v_accvgpr_"))
    print("v_mov_b32 %d on the walk, %d in the text; v_accvgpr_* %d / %d" % (moves, text_moves, acc, text_acc))
    assert moves <= PARENT_MOVES and text_moves <= PARENT_MOVES
    assert acc <= PARENT_ACCVGPR and text_acc <= PARENT_ACCVGPR
    assert sum(_count(walk, "v_mov_b64")) == 0


def test_the_iteration_is_shorter_by_the_pairs(walk):
    total = sum(len(ins) for ins in walk)
    nops = sum(_count(walk, "s_nop"))
    print("issued per layered iteration: %d (parent %d), %d of them s_nop" % (total, PARENT_ITERATION, nops))
    assert ITERATION <= PARENT_ITERATION - 12 * (PAIRS - 2)  # at least 22 of the 24 pairs per layer are net savings
    assert total <= ITERATION, total
    assert nops <= WAIT_STATES, nops
