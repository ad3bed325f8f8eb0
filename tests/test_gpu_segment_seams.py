"""GPU: the segmented sum (k_seg_sum / k_seg_fix / seg_fix_row of csrc/merlin_window.hip, through
merlin_segment_sum_fused and merlin_segment_sum_mask_rows) on key lists constructed to hold every seam of its
partition, with sources of small integers: every sum is exact in fp32 in any order (tests/fold_ref.py), so the output
must equal the float64 reference bit for bit.

Each named layout of fold_ref.layouts() asserts, from its entries alone, the seam classes it holds (items and their
ends, carry slots 0 and 1, fix rows spanning 1 .. 33 items, the 64-entry chunks and the two-chunk look-ahead, rounds
of 16 live entries, pairs split by a key change, dead chunks / items / keys, the second grid round at 8192 items).
Every layout runs with one and two towers, with and without a slot map (sub = 9), with no mask, a float mask, the
mask as bit words and the bit words read through mask_rows, and through both the fused launch and the two-launch
fix-up form; also accumulate onto a base, fill=False over a sentinel, and the marks."""
import pytest
import torch

import fold_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.mark.parametrize("use_slot", [False, True])
@pytest.mark.parametrize("name", R.NAMES)
def test_segment_sum_exact_on_layout(device, name, use_slot, monkeypatch):
    from merlin import _native as nat
    from merlin.windows import SegmentPlan

    c = R.seg_case(name, use_slot, device)
    plan = SegmentPlan(torch.from_numpy(c.keys).to(device), torch.from_numpy(c.idx).to(device), item_len=c.L)
    assert plan.nitems == (c.lay.n + c.L - 1) // c.L
    masks = {"none": {}, "float": {"mask": c.mask}, "words": {"mask": c.words},
             "words_rows": {"mask": c.words_rows, "mask_rows": c.mask_rows}}
    ar = torch.arange(c.nkeys, dtype=torch.int32, device=device)
    for T in (1, 2):
        src = c.src[:T].contiguous()
        base = R.ints((T, c.nkeys, 64), 77, -50, 50, device)
        for mname, mk in masks.items():
            kw = {k: (v[:T].contiguous() if k == "mask" else v) for k, v in mk.items()}
            ref = R.seg_ref(src, c.keys, c.idx, c.nkeys, slot=c.slot, sub=c.sub, item_len=c.L, **kw)
            R.assert_exact(ref.mag + 50)
            want = ref.out
            live = torch.zeros(c.nkeys, dtype=torch.bool, device=device)
            live[torch.tensor(sorted(ref.live), dtype=torch.int64, device=device)] = True
            dead_cross = torch.zeros_like(live)
            dc = sorted(ref.crossing - ref.live)
            dead_cross[torch.tensor(dc, dtype=torch.int64, device=device)] = True
            # fill=False over a sentinel: live keys hold the sums, dead crossing keys 0, every other key the sentinel
            want_nofill = torch.where((live | dead_cross)[None, :, None], want, torch.full_like(want, SENTINEL))
            want_mark = torch.where(live, ar, torch.full_like(ar, -1))
            for fused in (False, True):
                monkeypatch.setattr(nat, "SEG_FUSED", fused)
                tag = (name, use_slot, T, mname, fused)
                for _ in range(3 if fused else 2):
                    out = nat.segment_sum(src, plan, c.nkeys, slot=c.slot, sub=c.sub, **kw)
                    assert torch.equal(out.double(), want), (tag, float((out.double() - want).abs().max()))
                    if fused:
                        assert int(plan.counters.abs().sum()) == 0, tag
                acc = nat.segment_sum(src, plan, c.nkeys, slot=c.slot, sub=c.sub, out=base.clone(), accumulate=True, **kw)
                assert torch.equal(acc.double(), base.double() + want), tag
                mark = torch.full((c.nkeys,), -1, dtype=torch.int32, device=device)
                got = torch.full((T, c.nkeys, 64), SENTINEL, device=device)
                nat.segment_sum(src, plan, c.nkeys, slot=c.slot, sub=c.sub, out=got, fill=False, mark=mark, **kw)
                assert torch.equal(got.double(), want_nofill), tag
                assert torch.equal(mark, want_mark), tag
                if fused:
                    assert int(plan.counters.abs().sum()) == 0, tag
    if use_slot and name == "live_patterns":
        assert bool(dead_cross.any()) and bool((~live & ~dead_cross)[: c.nkeys - 1].any())
