"""CPU: the references and constructed cases of tests/fold_ref.py, which tests/test_gpu_head_seams.py and
tests/test_gpu_segment_seams.py hold the epilogue and segmented-sum kernels to.  Each reference on hand-computed
inputs; every named key-list layout holds the seam classes it claims (asserted from its entries alone); the builders
meet the exact-integer conditions (every sum of |terms| < 2^24, every row reaches an output, the towers differ);
merlin.windows.SegmentPlan, built on CPU tensors, equals a per-item restatement of its docstring on every layout."""
import numpy as np
import pytest
import torch

import fold_ref as R

NAN, INF = float("nan"), float("inf")


def t32(x):
    return torch.tensor(x, dtype=torch.float32)


def t64(x):
    return torch.tensor(x, dtype=torch.float64)


def test_bias_relu_by_hand():
    z = t32([[[1.0, -3.0, NAN, -0.0], [INF, -INF, 0.0, 2.0]]])
    b = t32([[1.0, 2.0, 5.0, -0.0]])
    ref = R.bias_relu(z, b)
    assert R.same(t32([[[2.0, 0.0, NAN, 0.0], [INF, 0.0, 5.0, 2.0]]]), ref)
    assert not R.same(t32([[[2.0, 0.0, 0.0, 0.0], [INF, 0.0, 5.0, 2.0]]]), ref)  # a NaN dropped
    assert not R.same(t32([[[2.0, 0.0, NAN, 0.0], [INF, 0.0, 5.0, 3.0]]]), ref)
    # -0.0 + b follows IEEE: -0.0 + -0.0 = -0.0 (relu: a zero of either sign), -0.0 + 3 = 3
    assert R.same(t32([[[0.0, 3.0]]]), R.bias_relu(t32([[[-0.0, -0.0]]]), t32([[-0.0, 3.0]])))


def test_relu_bwd_and_colsum_by_hand():
    y = t32([[[1.0, 0.0, -0.0, NAN], [-2.0, 3.0, 0.5, 4.0], [2.0, 2.0, NAN, -1.0]]])
    dy = t32([[[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [-9.0, 1.0, 1.0, 1.0]]])
    dz, db = R.relu_bwd(y, dy)
    assert torch.equal(dz, t64([[[1.0, 0, 0, 0], [0, 6.0, 7.0, 8.0], [-9.0, 1.0, 0, 0]]]))
    assert torch.equal(db, t64([[-8.0, 7.0, 7.0, 8.0]]))
    assert torch.equal(R.colsum(dy), t64([[-3.0, 9.0, 11.0, 13.0]]))
    x = torch.arange(2 * 3 * 2 * 4, dtype=torch.float32).view(2, 3, 2, 4)[:, :, 0]  # strided rows
    assert torch.equal(R.colsum(x), t64([[24.0, 27.0, 30.0, 33.0], [96.0, 99.0, 102.0, 105.0]]))


def test_head_bwd_and_heads_fwd_by_hand():
    # n = 2, H = 4, A = 2
    h = t32([[[1.0, 0.0, 2.0, -0.0], [0.0, 3.0, 1.0, 1.0]], [[2.0, 2.0, 0.0, 1.0], [1.0, 0.0, 0.0, 3.0]]])
    dl = t32([[1.0, -1.0], [2.0, 0.0]])
    dv = t32([3.0, -1.0])
    wa = t32([[1.0, 2.0, 3.0, 4.0], [0.0, 1.0, -1.0, 2.0]])
    wc = t32([1.0, -2.0, 5.0, 2.0])
    dz, db4, dWa, dwc = R.head_bwd(h, dl, dv, wa, wc)
    # tower 0: g = dl Wa = [[1, 1, 4, 2], [2, 4, 6, 8]]; tower 1: g = dv wc = [[3, -6, 15, 6], [-1, 2, -5, -2]]
    assert torch.equal(dz, t64([[[1.0, 0, 4.0, 0], [0, 4.0, 6.0, 8.0]], [[3.0, -6.0, 0, 6.0], [-1.0, 0, 0, -2.0]]]))
    assert torch.equal(db4, t64([[1.0, 4.0, 10.0, 8.0], [2.0, -6.0, 0.0, 4.0]]))
    assert torch.equal(dWa, t64([[1.0, 6.0, 4.0, 2.0], [-1.0, 0.0, -2.0, 0.0]]))
    assert torch.equal(dwc, t64([5.0, 6.0, 0.0, 0.0]))
    h5 = torch.zeros(2, 2, 512)
    h5[0, 0, 0], h5[0, 0, 511], h5[0, 1, 256], h5[1, 0, 3], h5[1, 1, 3] = 2.0, 3.0, 1.0, 4.0, -1.0
    wa5, wc5 = torch.zeros(2, 512), torch.zeros(512)
    wa5[0, 0], wa5[0, 511], wa5[1, 256], wc5[3] = 1.0, -1.0, 7.0, 2.0
    lg, v = R.heads_fwd(h5, wa5, wc5)
    assert torch.equal(lg, t64([[-1.0, 0.0], [0.0, 7.0]])) and torch.equal(v, t64([8.0, -2.0]))
    lg, v = R.heads_fwd(h5, wa5, wc5, t32([1.0, 2.0]), t32([10.0]))
    assert torch.equal(lg, t64([[0.0, 2.0], [1.0, 9.0]])) and torch.equal(v, t64([18.0, 8.0]))


def test_seg_ref_by_hand():
    # four rows of 64 columns: row r holds r + 1 at every column; two keys
    src = (torch.arange(4, dtype=torch.float32) + 1)[None, :, None].expand(1, 4, 64).contiguous()
    keys, idx = np.array([0, 0, 2, 2, 2]), np.array([3, 0, 1, 1, 2])
    r = R.seg_ref(src, keys, idx, 4, item_len=2)
    assert torch.equal(r.out[0, :, 0], t64([5.0, 0.0, 7.0, 0.0])) and r.live == {0, 2} and r.crossing == {2}
    # slot map over frames of two rows: frame 0 dead, frame 1 -> slot 0: ids 2, 3 -> rows 0, 1
    slot = torch.tensor([-1, 0], dtype=torch.int32)
    r = R.seg_ref(src[:, :2].contiguous(), keys, idx, 4, slot=slot, sub=2)
    assert torch.equal(r.out[0, :, 5], t64([2.0, 0.0, 1.0, 0.0])) and r.live == {0, 2}
    # masks: column 0 open on rows 0 and 2 only; NaN, -0.0 and negatives close a column
    mask = torch.full((1, 4, 64), -1.0)
    mask[0, 0, 0], mask[0, 2, 0], mask[0, 1, 0], mask[0, 3, 0], mask[0, 1, 63] = 1.0, 0.5, NAN, -0.0, 2.0
    r = R.seg_ref(src, keys, idx, 4, mask=mask)
    assert torch.equal(r.out[0, :, 0], t64([1.0, 0.0, 3.0, 0.0])) and torch.equal(r.out[0, :, 63], t64([0.0, 0, 4.0, 0]))
    words = R.words_of(mask)
    assert words.tolist() == [[1, -(1 << 63), 1, 0]]
    assert torch.equal(R.bits_of(words), mask > 0)
    assert torch.equal(R.seg_ref(src, keys, idx, 4, mask=words).out, r.out)
    mrow = torch.tensor([2, 0, 3, 1], dtype=torch.int32)
    scattered = torch.empty_like(words)
    scattered[:, mrow.long()] = words
    assert torch.equal(R.seg_ref(src, keys, idx, 4, mask=scattered, mask_rows=mrow).out, r.out)
    assert R.crossing_keys([0, 0, 1, 1, 2, 2], 2) == set() and R.crossing_keys([0, 1, 1, 1, 1, 2], 2) == {1}


def test_seam_classes_by_hand():
    keys, live = R.expand([(0, 3), (1, 5, "x.x.."), (4, 4, "D")])
    assert keys.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 4, 4, 4, 4] and live.tolist() == [True] * 4 + [False, True] + [False] * 6
    got = R.seam_classes(keys, live, 4)
    assert {"nnz_kL", "carry1", "span1", "abut", "dead_key_no_cross", "odd_pair_change"} <= got
    assert not got & {"carry0", "span2", "nnz_kL1", "abut_only", "dead_key_crossing"}
    got = R.seam_classes(*R.expand([(0, 9, "D"), (1, 1)]), 4)
    assert {"carry0", "span2", "whole_interior", "dead_key_crossing", "dead_item_crossing"} <= got
    with pytest.raises(AssertionError):
        R.expand([(1, 2), (1, 3)])  # keys must ascend
    assert R.plan_ref([0, 0, 0, 1, 1, 1, 1, 1, 4, 4, 4, 4], 4) == ([(1, 0, 1, 1), (-1, 1, -1, -1), (-1, 2, -1, -1)], [-1, 0, -1])
    assert R.plan_ref([7] * 9, 4) == ([(7, 0, 2, 0), (-1, 1, -1, -1), (-1, 2, -1, -1)], [-1, 0, 0])


@pytest.mark.parametrize("name", R.NAMES)
def test_layout_holds_its_classes_and_plan(name):
    from merlin.windows import SegmentPlan

    lay = R.layout(name)  # asserts the classes
    assert lay.n == len(lay.live) and lay.nkeys > int(lay.keys.max()) + 1  # one key past the last is never named
    keys = torch.from_numpy(lay.keys)
    plan = SegmentPlan(keys, torch.zeros_like(keys), item_len=lay.L)
    fix, head = R.plan_ref(lay.keys, lay.L)
    assert plan.nitems == len(fix) and plan.fix.shape == (len(fix), 4) and plan.fix.dtype == torch.int32
    got = plan.fix.tolist()
    for j, (want, g) in enumerate(zip(fix, got)):
        assert g[0] == want[0], (j, g, want)
        if want[0] >= 0:
            assert tuple(g) == want, (j, g, want)
    assert plan.head_fix.tolist() == head
    assert plan.counters.shape == (len(fix),) and int(plan.counters.abs().sum()) == 0
    # the fix rows name exactly the crossing keys
    assert {w[0] for w in fix if w[0] >= 0} == R.crossing_keys(lay.keys, lay.L)


def test_layouts_cover_every_class():
    got = set()
    for name in R.NAMES:
        got |= R.layout(name).classes
    want = {"nnz1", "nnz_lt_L", "nnz_kL", "nnz_kL1", "last63", "last64", "last65", "abut", "abut_only", "carry0", "carry1",
            "whole_interior", "both_cross_direct", "two_keys_both_cross", "odd_pair_change", "change_after_16",
            "dead_chunk_in_run", "dead_item_crossing", "dead_key_no_cross", "dead_key_crossing", "nitems8191",
            "nitems8192", "nitems8193"}
    want |= {"span%d" % s for s in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)}
    want |= {"change@%d" % o for o in (63, 64, 65, 127, 128, 129)}
    want |= {"chunk_live%d" % c for c in (0, 1, 15, 16, 17, 63)}
    assert want <= got, sorted(want - got)


@pytest.mark.parametrize("name", ["kL", "carries", "live_patterns", "chunk_edges64"])
@pytest.mark.parametrize("use_slot", [False, True])
def test_seg_case_conditions(name, use_slot):
    c = R.seg_case(name, use_slot)
    ref = R.seg_ref(c.src, c.keys, c.idx, c.nkeys, slot=c.slot, sub=c.sub, item_len=c.L)
    R.assert_exact(ref.mag)
    assert ref.live == set(int(k) for k in np.unique(c.keys[c.live_entries]))
    assert len(set(ref.rows.tolist())) == len(ref.rows)  # every live entry has a source row of its own
    assert int(ref.rows.max()) < c.src.shape[1] and int(ref.rows.min()) >= 0
    if use_slot and name == "live_patterns":
        assert ref.live != set(int(k) for k in np.unique(c.keys))  # there are dead keys
    # the three mask forms agree, and the mask leaves every row visible
    a = R.seg_ref(c.src, c.keys, c.idx, c.nkeys, slot=c.slot, sub=c.sub, mask=c.mask)
    b = R.seg_ref(c.src, c.keys, c.idx, c.nkeys, slot=c.slot, sub=c.sub, mask=c.words)
    d = R.seg_ref(c.src, c.keys, c.idx, c.nkeys, slot=c.slot, sub=c.sub, mask=c.words_rows, mask_rows=c.mask_rows)
    assert torch.equal(a.out, b.out) and torch.equal(a.out, d.out) and not torch.equal(a.out, ref.out)
    assert bool(torch.isnan(c.mask).any()) and bool((c.mask == 0).any()) and bool((c.mask < 0).any())
    assert not torch.equal(c.words, c.words_rows)


def test_epilogue_builders_meet_the_conditions():
    for rows, cols in ((1, 4), (33, 64), (257, 512), (65, 1024)):
        y, dy = R.relu_case(2, rows, cols, 3)
        assert y.shape == dy.shape == (2, rows, cols)
        if rows * cols >= 2048:
            assert bool(torch.isnan(y).any()) and bool((y < 0).any())
            assert bool(((y == 0) & torch.signbit(y)).any()) and bool(((y == 0) & ~torch.signbit(y)).any())
        x = R.colsum_case(2, rows, cols, 4)
        assert x.is_contiguous()
    x = R.colsum_case(2, 33, 64, 5, taps=9)
    assert x.shape == (2, 33, 64) and x.stride() == (33 * 576, 576, 1)
    z, b = R.bias_relu_case(2, 4097, 64, 6)
    assert bool(torch.isnan(z).any()) and bool(torch.isinf(z).any()) and bool(((z == 0) & torch.signbit(z)).any())
    for n, H, A in ((1, 512, 3), (65, 512, 8), (33, 4, 2), (129, 64, 1), (33, 1024, 3)):
        h, dl, dv, wa, wc = R.head_case(n, H, A, 7)
        assert h.shape == (2, n, H) and dl.shape == (n, A) and wa.shape == (A, H) and bool((h >= 0).all())
    for A, bias in ((1, True), (8, False)):
        R.heads_fwd_case(17, A, bias, 8)
    with pytest.raises(AssertionError):
        R.assert_exact(t64([2.0 ** 24]))
    R.assert_exact(t64([2.0 ** 24 - 1]))
    assert R.ints((1000,), 1, -3, 3).unique().tolist() == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    assert R.nonzero_ints((1000,), 1, 2).unique().tolist() == [-2.0, -1.0, 1.0, 2.0]
    assert not torch.equal(R.ihash((64,), 1), R.ihash((64,), 2))
