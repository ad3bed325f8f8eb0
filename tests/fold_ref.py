"""The fold tests' own references and constructed cases (no test in here, no GPU code; plain torch / numpy):

  * the tower epilogues of csrc/merlin_head.hip restated in float64 from the formulas of its header comments
    (bias_relu, relu_bwd, colsum, head_bwd, heads_fwd),
  * the segmented sum of csrc/merlin_window.hip (seg_ref: out[t][k] = the sum over the entries with key k of the
    source rows they name, through the slot map and any of the three mask forms),
  * builders of inputs made of small integers, and named key-list layouts that put a run on every seam of the
    segmented sum's partition (items, 64-entry chunks, rounds of 16 live entries, pairs, carries, fix rows).

The exact-integer rule.  Every value is a small integer stored as fp32, so every product and every partial sum of a
case is an integer; each builder asserts that the largest sum of |terms| of any output is below 2^24, so all of them
are exact in fp32 IN ANY ORDER.  A kernel's output must then equal the float64 reference bit for bit (torch.equal
after the cast): there is no tolerance, and a dropped, doubled or misrouted row moves a sum by at least 1.  Each
builder also asserts that every row contributes a non-zero (after the mask) to at least one output, so the loss of
any single row shows.

Special values.  bias_relu: v = z + b in IEEE arithmetic (-0.0 + b = b, +-inf + b = +-inf), then NaN stays NaN and
everything else becomes max(v, 0); a zero result compares equal whatever its sign (the kernel's fmaxf may return
either zero for max(-0.0, 0.0)).  relu_bwd: dz = dy where y > 0, else +0: y = +0.0, -0.0, negatives and NaN all
give 0.  `same` is the comparison: the NaN positions agree and every other element is equal by value."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

LIMIT = float(2 ** 24)


# ----------------------------------------------------------------------------------------------------------------------
# Values: a fixed integer hash of the flat element index (any device), so the large cases cost no host generation.
def ihash(shape, seed, device="cpu"):
    """int64 tensor of `shape`, well mixed values in [0, 2^16) from the flat index and the seed."""
    n = int(np.prod(shape))
    x = (torch.arange(n, dtype=torch.int64, device=device) + (int(seed) + 1) * 0x9E3779B1) & 0xFFFFFFFF
    for _ in range(2):
        x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    return ((x >> 8) & 0xFFFF).view(*shape)


def ints(shape, seed, lo, hi, device="cpu"):
    """fp32 integers in [lo, hi]."""
    return (ihash(shape, seed, device) % (hi - lo + 1) + lo).float()


def nonzero_ints(shape, seed, m, device="cpu"):
    """fp32 integers in [-m, m] without 0."""
    v = ihash(shape, seed, device) % (2 * m)
    return torch.where(v < m, v - m, v - m + 1).float()


def same(got, ref):
    """got (fp32) == ref (float64) element for element: NaN where and only where ref is NaN, equal values elsewhere."""
    g = got.double()
    gn, rn = torch.isnan(g), torch.isnan(ref)
    z = torch.zeros((), dtype=torch.float64, device=g.device)
    return bool(torch.equal(gn, rn)) and bool(torch.equal(torch.where(gn, z, g), torch.where(rn, z, ref)))


def assert_exact(abs_sum):
    """The exact-integer condition: the largest sum of |terms| of any output is below 2^24."""
    m = float(abs_sum.max()) if abs_sum.numel() else 0.0
    assert m < LIMIT, m


# ----------------------------------------------------------------------------------------------------------------------
# Epilogue references (float64, on the device of their inputs).
def bias_relu(z, b):
    """relu(z[t][r][:] + b[t][:]) with NaN kept (see the module docstring)."""
    v = z.double() + b.double()[:, None]
    return torch.where(torch.isnan(v), v, v.clamp_min(0.0))


def relu_bwd(y, dy):
    """(dz, dbias): dz = [y > 0] * dy, dbias[t][c] = sum_r dz[t][r][c]."""
    dz = torch.where(y > 0, dy.double(), torch.zeros((), dtype=torch.float64, device=y.device))
    return dz, dz.sum(1)


def colsum(x):
    return x.double().sum(1)


def head_bwd(h, dlogits, dvalue, wa, wc):
    """(dz [2, n, H], db4 [2, H], dWa [A, H], dwc [H]) of the heads on h = relu(fc1):
    dz[0][k] = [h0 > 0] * sum_j dlogits[k][j] Wa[j],  dz[1][k] = [h1 > 0] * dvalue[k] wc,
    db4[t] = sum_k dz[t][k],  dWa[j] = sum_k dlogits[k][j] h0[k],  dwc = sum_k dvalue[k] h1[k]."""
    h64, dl, dv = h.double(), dlogits.double(), dvalue.double().reshape(-1)
    wa64, wc64 = wa.double(), wc.double().reshape(-1)
    g = torch.stack([dl @ wa64, dv[:, None] * wc64[None]])
    dz = torch.where(h > 0, g, torch.zeros((), dtype=torch.float64, device=h.device))
    return dz, dz.sum(1), dl.t() @ h64[0], dv @ h64[1]


def heads_fwd(h, wa, wc, ba=None, bc=None):
    """(logits [n, A], value [n]): h[0] Wa^T (+ ba), h[1] wc (+ bc)."""
    h64 = h.double()
    logits = h64[0] @ wa.double().t()
    value = h64[1] @ wc.double().reshape(-1)
    if ba is not None:
        logits = logits + ba.double()
    if bc is not None:
        value = value + bc.double().reshape(-1)
    return logits, value


# ----------------------------------------------------------------------------------------------------------------------
# Epilogue cases.
def relu_pattern(shape, seed, device="cpu"):
    """A forward output for the ReLU backward / a ReLU mask: +0.0, -0.0, negatives, a few NaN, positives; row r of
    every tower is positive at column r % cols."""
    T, rows, cols = shape
    code = ihash(shape, seed, device) % 64
    y = (code - 30).float()                                    # 31..63 -> 1..33
    y = torch.where(code < 31, -(code - 16).float(), y)        # 17..30 -> -1..-14
    y = torch.where(code < 17, torch.full_like(y, -0.0), y)    # 9..16
    y = torch.where(code < 9, torch.zeros_like(y), y)          # 1..8
    y = torch.where(code == 0, torch.full_like(y, float("nan")), y)
    rr = torch.arange(rows, device=device)
    y[:, rr, rr % cols] = 1.0 + (rr % 3).float()
    return y


def relu_case(T, rows, cols, seed, device="cpu"):
    """y, dy [T, rows, cols] for relu_bwd; every row passes a non-zero at column r % cols."""
    y = relu_pattern((T, rows, cols), seed, device)
    dy = ints((T, rows, cols), seed + 1, -3, 3, device)
    rr = torch.arange(rows, device=device)
    dy[:, rr, rr % cols] = 1.0 + (rr % 2).float()
    dz = torch.where(y > 0, dy, torch.zeros_like(dy))
    assert_exact(dz.double().abs().sum(1))
    assert bool((dz != 0).any(2).all())  # every row reaches a column sum
    if T == 2:
        assert not torch.equal(dy[0], dy[1]) or rows * cols < 8
    return y, dy


def colsum_case(T, rows, cols, seed, device="cpu", taps=None):
    """x [T, rows, cols] of integers, every row non-zero; with taps, the strided view [:, :, 0] of [T, rows, taps,
    cols]."""
    full = (T, rows, cols) if taps is None else (T, rows, taps, cols)
    big = ints(full, seed, -4, 4, device)
    x = big if taps is None else big[:, :, 0]
    rr = torch.arange(rows, device=device)
    x[:, rr, rr % cols] = 1.0 + (rr % 4).float()
    assert_exact(x.double().abs().sum(1))
    assert bool((x != 0).any(2).all())
    return x


def bias_relu_case(T, rows, cols, seed, device="cpu"):
    """z [T, rows, cols], b [T, cols]: integers with NaN, +-inf and -0.0 among z and +0.0, -0.0 among b."""
    code = ihash((T, rows, cols), seed, device) % 97
    z = (code % 9 - 4).float()
    for c, v in ((93, float("nan")), (94, float("inf")), (95, float("-inf")), (96, -0.0)):
        z = torch.where(code == c, torch.full_like(z, v), z)
    b = ints((T, cols), seed + 1, -2, 2, device)
    b[:, 1] = -0.0
    b[:, 2] = 0.0
    return z, b


def head_case(n, H, A, seed, device="cpu"):
    """h [2, n, H] >= 0 (relu outputs: +0.0, -0.0, 1..3), dlogits [n, A], dvalue [n], wa [A, H], wc [H]: small
    integers such that the head gradient of every row is non-zero at every column (dlogits[r] = s_r * m_r with m_r >= 0
    not all zero, Wa[j][k] = g_k * p_jk with p > 0: the sum over j cannot cancel), so every row reaches db4, dWa and
    dwc through the column r % H at which its h is positive."""
    code = ihash((2, n, H), seed, device) % 8
    h = (code - 4).float().clamp_min(0.0)                    # 5, 6, 7 -> 1, 2, 3
    h = torch.where(code == 0, torch.full_like(h, -0.0), h)
    rr = torch.arange(n, device=device)
    h[:, rr, rr % H] = 1.0 + (rr % 3).float()
    m = ints((n, A), seed + 1, 0, 2, device)
    m[rr, rr % A] = 1.0 + (rr % 2).float()
    s = nonzero_ints((n, 1), seed + 2, 1, device)
    dlogits = s * m
    dvalue = nonzero_ints((n,), seed + 3, 2, device)
    wa = nonzero_ints((1, H), seed + 4, 1, device) * ints((A, H), seed + 5, 1, 2, device)
    wc = nonzero_ints((H,), seed + 6, 2, device)
    dz, _, _, _ = head_bwd(h, dlogits, dvalue, wa, wc)
    assert_exact(dz.abs().sum(1))
    assert_exact(dlogits.double().abs().t() @ h.double()[0])
    assert_exact(dvalue.double().abs() @ h.double()[1])
    assert bool((dz != 0).any(2).all())                                       # every row reaches db4
    assert bool(((dlogits != 0).any(1) & (h[0] != 0).any(1)).all())          # ... dWa
    assert bool(((dvalue != 0) & (h[1] != 0).any(1)).all())                  # ... dwc
    assert not torch.equal(h[0], h[1]) or n * H < 8
    return h, dlogits, dvalue, wa, wc


def heads_fwd_case(n, A, bias, seed, device="cpu"):
    """h [2, n, 512] >= 0, wa [A, 512], wc [512] (and ba [A], bc [1]): integers; every dot product stays below 2^24."""
    h = ints((2, n, 512), seed, 0, 3, device)
    wa = ints((A, 512), seed + 1, -2, 2, device)
    wc = ints((512,), seed + 2, -2, 2, device)
    ba = ints((A,), seed + 3, -5, 5, device) if bias else None
    bc = ints((1,), seed + 4, 3, 7, device) if bias else None
    assert_exact(h.double()[0].abs() @ wa.double().abs().t() + 5)
    assert_exact(h.double()[1].abs() @ wc.double().abs() + 7)
    assert not torch.equal(h[0], h[1]) or n < 2
    return h, wa, wc, ba, bc


# ----------------------------------------------------------------------------------------------------------------------
# The segmented sum.
def words_of(mask):
    """The bit-word form of a float mask [T, rows, 64] (bit c of word [t][r] = mask[t][r][c] > 0), built on the host:
    int64 [T, rows]."""
    m = (mask.detach().cpu() > 0).numpy().astype(np.uint64)
    w = (m << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return torch.from_numpy(w.view(np.int64).copy())


def bits_of(words):
    """bool [T, rows, 64] of int64 bit words."""
    sh = torch.arange(64, dtype=torch.int64, device=words.device)
    return ((words.unsqueeze(-1) >> sh) & 1).bool()


def seg_ref(src, keys, idx, nkeys, slot=None, sub=1, mask=None, mask_rows=None, item_len=None):
    """out float64 [T, nkeys, 64]: out[t][k] = the sum over the entries e with keys[e] == k, in list order, of
    src[t][row(e)] (times [mask > 0] of that row: a float mask of src's shape, int64 bit words [T, rows], or bit words
    read through mask_rows: row r's word is mask[t][mask_rows[r]]); row(e) = idx[e], or slot[idx[e] // sub] * sub +
    idx[e] % sub with the entries whose slot is -1 skipped.  Also returned: `live`, the keys that have an entry not
    skipped, and (with item_len) `crossing`, the keys with entries on both sides of an item end -- found by a literal
    loop over the items."""
    dev = src.device
    keys_t = torch.as_tensor(np.asarray(keys), dtype=torch.int64, device=dev)
    idx_t = torch.as_tensor(np.asarray(idx), dtype=torch.int64, device=dev)
    if slot is not None:
        s = slot.to(dev).long()[idx_t // sub]
        keep = s >= 0
        rows, kk = (s * sub + idx_t % sub)[keep], keys_t[keep]
    else:
        rows, kk = idx_t, keys_t
    x = src.double()
    if mask is not None:
        if mask.dtype == torch.int64:
            b = bits_of(mask)
            if mask_rows is not None:
                b = b[:, mask_rows.to(dev).long()]
        else:
            b = mask > 0
        x = torch.where(b, x, torch.zeros((), dtype=torch.float64, device=dev))
    T = int(src.shape[0])
    out = torch.zeros(T, nkeys, 64, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(out)
    # the list is sorted by key, so a key's sum is a difference of running sums over the entries (exact in float64
    # for the integer cases; an index_add_ of thirty thousand rows onto one key is a queue of float64 atomics)
    assert bool((kk[1:] >= kk[:-1]).all())
    uniq, counts = torch.unique_consecutive(kk, return_counts=True)
    ends = counts.cumsum(0)
    for t in range(T):
        for dst, v in ((out, x[t, rows]), (mag, x[t, rows].abs())):
            cs = torch.cat([torch.zeros(1, 64, dtype=torch.float64, device=dev), v.cumsum(0)])
            dst[t, uniq] = cs[ends] - cs[ends - counts]
    live = set(int(k) for k in uniq.cpu().tolist())
    crossing = None
    if item_len is not None:
        crossing = crossing_keys(keys, item_len)
    return SimpleNamespace(out=out, mag=mag, live=live, crossing=crossing, rows=rows, kk=kk)


def crossing_keys(keys, L):
    """The keys that have entries in two neighbouring items, by a literal loop over the items."""
    keys = [int(k) for k in keys]
    n, out = len(keys), set()
    nitems = (n + L - 1) // L
    for j in range(nitems):
        last = min((j + 1) * L, n) - 1
        if last + 1 < n and keys[last + 1] == keys[last]:
            out.add(keys[last])
    return out


def plan_ref(keys, L):
    """SegmentPlan's fix rows and head_fix, restated per item from its docstring: fix[j] = (dst, j, last item of dst's
    run, carry slot) for the destination that starts in item j and continues past it (carry slot 0 when it starts on
    the item's first entry, else 1), dst = -1 when there is none; head_fix[j] = the item in which item j's first
    destination started when it started before the item, else -1."""
    keys = [int(k) for k in keys]
    n = len(keys)
    nitems = (n + L - 1) // L
    fix, head = [], []
    for j in range(nitems):
        e0, e1 = j * L, min((j + 1) * L, n)
        k = keys[e1 - 1]
        s = e1 - 1
        while s > 0 and keys[s - 1] == k:
            s -= 1
        e = e1
        while e < n and keys[e] == k:
            e += 1
        if e > e1 and s >= e0:
            fix.append((k, j, (e - 1) // L, 0 if s == e0 else 1))
        else:
            fix.append((-1, j, -1, -1))
        kf = keys[e0]
        s = e0
        while s > 0 and keys[s - 1] == kf:
            s -= 1
        head.append(s // L if s < e0 else -1)
    return fix, head


# -- layouts -----------------------------------------------------------------------------------------------------------
# A layout is an item length and a list of runs (key, length, live pattern) in entries; keys ascend.  The live pattern
# says which entries of the run survive a slot map ("L" all, "D" none, ("mod", m, r): entry i is dead when i % m == r,
# or an explicit string of 'x' / '.' = live / dead); without a slot map every entry is live.
CHUNK, ROUND = 64, 16  # k_seg_sum: entries loaded per step of an item, live entries per unrolled round (8 pairs)


def _pattern(p, n):
    if p == "L":
        return np.ones(n, dtype=bool)
    if p == "D":
        return np.zeros(n, dtype=bool)
    if isinstance(p, tuple):
        return np.arange(n) % p[1] != p[2]
    assert len(p) == n, (p, n)
    return np.array([c == "x" for c in p])


def expand(runs):
    """(keys int64 [n], live bool [n]) of a run list."""
    ks = [r[0] for r in runs]
    assert all(a < b for a, b in zip(ks[:-1], ks[1:])), "keys must ascend"
    keys = np.concatenate([np.full(r[1], r[0], dtype=np.int64) for r in runs])
    live = np.concatenate([_pattern(r[2] if len(r) > 2 else "L", r[1]) for r in runs])
    return keys, live


def seam_classes(keys, live, L):
    """The set of seam classes a key list holds, from its entries alone (the table in DESIGN.md, section 4)."""
    keys, live = np.asarray(keys), np.asarray(live)
    n = len(keys)
    nitems = (n + L - 1) // L
    out = set()
    # a: list length against the item length
    if n == 1:
        out.add("nnz1")
    if n < L:
        out.add("nnz_lt_L")
    if n >= L and n % L == 0:
        out.add("nnz_kL")
    if n > L and n % L == 1:
        out.add("nnz_kL1")
    if L == 1024 and nitems > 1 and n - (nitems - 1) * L in (63, 64, 65):
        out.add("last%d" % (n - (nitems - 1) * L))
    if L == 4 and nitems in (8191, 8192, 8193):
        out.add("nitems%d" % nitems)  # m
    # runs
    starts = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    ends = np.concatenate([starts[1:], [n]])
    crosses = False
    for s, e in zip(starts, ends):
        s, e = int(s), int(e)
        j0, j1 = s // L, (e - 1) // L
        if j1 > j0:
            crosses = True
            out.add("carry0" if s % L == 0 else "carry1")                      # c
            out.add("span%d" % (j1 - j0))                                       # d
            if j1 - j0 >= 2:
                out.add("whole_interior")  # items j0 + 1 .. j1 - 1 hold this key alone
            if not live[s:e].any():
                out.add("dead_key_crossing")
        elif not live[s:e].any():
            out.add("dead_key_no_cross")                                        # l
    # b: item ends on which one run stops and the next begins
    edges = [p for p in range(L, n, L)]
    if any(keys[p - 1] != keys[p] for p in edges):
        out.add("abut")
    if edges and not crosses:
        out.add("abut_only")
    for j in range(nitems):
        e0, e1 = j * L, min((j + 1) * L, n)
        k = keys[e0:e1]
        xfirst = e0 > 0 and keys[e0 - 1] == k[0]
        xlast = e1 < n and keys[e1] == k[-1]
        nk = len(np.unique(k))
        if xfirst and xlast and nk >= 3:
            out.add("both_cross_direct")                                        # e
        if xfirst and xlast and nk == 2:
            out.add("two_keys_both_cross")
        if not live[e0:e1].any() and (xfirst or xlast):
            out.add("dead_item_crossing")                                       # k
        if L == 1024:
            for o in (63, 64, 65, 127, 128, 129):                               # f
                if e0 + o < e1 and keys[e0 + o] != keys[e0 + o - 1]:
                    out.add("change@%d" % o)
        for c0 in range(e0, e1, CHUNK):
            c1 = min(c0 + CHUNK, e1)
            lv = np.flatnonzero(live[c0:c1]) + c0
            if c1 - c0 == CHUNK and len(lv) in (0, 1, 15, 16, 17, 63):
                out.add("chunk_live%d" % len(lv))                               # g
            kl = keys[lv]
            for i in range(1, len(lv)):
                if kl[i] != kl[i - 1]:
                    if i % 2 == 1:
                        out.add("odd_pair_change")                              # h
                    if i % ROUND == 0:
                        out.add("change_after_16")                              # i
            if len(lv) == 0 and c0 > e0 and c1 < e1 and keys[c0 - 1] == keys[c1] and live[e0:c0][keys[e0:c0] == keys[c1]].any() \
                    and live[c1:e1][keys[c1:e1] == keys[c1]].any():
                out.add("dead_chunk_in_run")                                    # j
    return out


def _spans(L, first):
    spans = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)
    runs, k = [], 0
    if not first:
        runs.append((k, L // 2, ("mod", 3, 1)))  # every following run starts mid-item: carry slot 1
        k += 2
    for s in spans:
        if first:  # starts on an item's first entry, ends 5 entries into item j0 + s; a direct run fills the item
            runs += [(k, L * s + 5, ("mod", 7, 2)), (k + 1, L - 5, "L")]
        else:
            runs.append((k, L * s, ("mod", 5, 0)))
        k += 3
    return runs


def _chunk_edges(tail):
    # key changes at entries 63, 64, 65, 127, 128, 129 of item 0 (L = 1024); the last item holds `tail` entries
    return [(0, 63, ("mod", 4, 1)), (1, 1), (2, 1), (3, 62, ("mod", 3, 0)), (4, 1), (6, 1), (7, 895 + tail - 10, ("mod", 6, 5)),
            (9, 10, "L")]


def _live_patterns():
    # L = 256, four 64-entry chunks per item
    x, d = "x", "."
    return [
        (0, 64, "D"),                                            # item 0 chunk 0: no live entry; key 0 dead, no crossing
        (1, 64, d * 6 + x + d * 57),                             # chunk 1: 1 live
        (2, 64, x * 15 + d * 49),                                # chunk 2: 15 live
        (3, 30, (x + d) * 14 + x * 2), (4, 34, "D"),             # chunk 3: 16 live; key 4 dead
        (5, 64, (x * 2 + d) * 8 + x + d * 39),                   # item 1 chunk 0: 17 live
        (6, 192, x * 63 + d + d * 64 + x * 64),                  # chunks 1-3: 63 live, a dead chunk inside the run, 64 live
        (7, 4, x + d + x * 2), (8, 60, (x + d) * 30),            # item 2 chunk 0: key change at live offset 3 (odd)
        (9, 20, x * 4 + d * 2 + x * 10 + d * 2 + x * 2),         # chunk 1: 16 live of key 9 ...
        (10, 44, "L"),                                           # ... then key 10 from live offset 16
        (11, 128 + 256 + 10, x * 128 + d * 256 + x * 10),        # chunks 2-3, ALL of item 3 dead, 10 live in item 4
        (12, 236, ("mod", 4, 2)),
        (13, 20, "D"),                                           # dead key crossing from item 4 into item 5
        (15, 30, "L"),
    ]


def _grid_round(nitems):
    # L = 4: runs of 3, 5, 1, 7, 2, 6, 4, 9 entries over and over (most cross an item end), 4 * nitems - 1 entries
    n, cyc, runs, k, i = 4 * nitems - 1, (3, 5, 1, 7, 2, 6, 4, 9), [], 0, 0
    while n > 0:
        m = min(n, cyc[i % 8])
        runs.append((k, m, ("mod", 5, 3)))
        n -= m
        k += 1 + (i % 3 == 0)
        i += 1
    return runs


def layouts():
    """name -> (item length, runs, the classes the layout must hold)."""
    out = {
        "one": (4, [(2, 1)], {"nnz1", "nnz_lt_L"}),
        "short": (1024, [(1, 3, "x.x"), (4, 2)], {"nnz_lt_L"}),
        "kL": (4, [(0, 3), (1, 5, "x.xx."), (3, 4)], {"nnz_kL", "carry1"}),
        "kL1": (4, [(0, 3), (1, 5), (3, 5, ".xxxx")], {"nnz_kL1", "carry0"}),
        "abut": (64, [(0, 64, ("mod", 3, 0)), (1, 64), (3, 30, ("mod", 2, 0)), (4, 34), (6, 64, ("mod", 9, 8))],
                 {"abut", "abut_only", "nnz_kL"}),
        "carries": (64, [(0, 74, ("mod", 4, 1)), (1, 40), (2, 30, ("mod", 3, 2)), (3, 48, ("mod", 5, 0))],
                    {"carry0", "carry1", "span1"}),
        "spans_mid": (16, _spans(16, False), {"carry1", "whole_interior"} | {"span%d" % s for s in
                                                                            (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)}),
        "spans_first": (64, _spans(64, True), {"carry0", "whole_interior"} | {"span%d" % s for s in
                                                                              (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)}),
        "span33_1024": (1024, [(0, 500, ("mod", 7, 0)), (1, 33 * 1024, ("mod", 11, 4)), (3, 100)],
                        {"span33", "carry1", "whole_interior"}),
        "both_cross": (64, [(0, 70, ("mod", 3, 1)), (1, 10), (2, 20, ("mod", 2, 1)), (3, 58, ("mod", 4, 0)),
                            (5, 74, ("mod", 5, 2)), (6, 44, ("mod", 3, 0)), (7, 44)],
                       {"both_cross_direct", "two_keys_both_cross", "carry0", "carry1"}),
        "live_patterns": (256, _live_patterns(),
                          {"chunk_live0", "chunk_live1", "chunk_live15", "chunk_live16", "chunk_live17", "chunk_live63",
                           "odd_pair_change", "change_after_16", "dead_chunk_in_run", "dead_item_crossing",
                           "dead_key_no_cross", "dead_key_crossing"}),
    }
    for tail in (63, 64, 65):
        out["chunk_edges%d" % tail] = (1024, _chunk_edges(tail), {"last%d" % tail, "carry1"} | {
            "change@%d" % o for o in (63, 64, 65, 127, 128, 129)})
    for nitems in (8191, 8192, 8193, 8200):
        want = {"nitems%d" % nitems} if nitems < 8200 else set()
        out["grid%d" % nitems] = (4, _grid_round(nitems), want | {"carry0", "carry1", "span1", "span2"})
    return out


NAMES = tuple(layouts())
SUB = 9  # rows per frame of the slot-mapped cases (the update's nine conv3 positions)


@lru_cache(maxsize=None)
def layout(name):
    """The checked layout: L, keys, live (numpy), nkeys, and its classes -- asserted from the entries alone."""
    L, runs, want = layouts()[name]
    keys, live = expand(runs)
    got = seam_classes(keys, live, L)
    assert want <= got, (name, sorted(want - got))
    if name == "abut":
        assert not crossing_keys(keys, L)
    if name.startswith("grid"):
        assert (len(keys) + L - 1) // L == int(name[4:])
    return SimpleNamespace(name=name, L=L, keys=keys, live=live, nkeys=int(keys.max()) + 2, classes=got, n=len(keys))


def seg_case(name, use_slot, device="cpu", seed=0):
    """The inputs of one segmented-sum case (T = 2; a T = 1 run takes the first tower):

      keys, idx (numpy int64, list order), slot (int32 [F] or None), sub, nkeys, L,
      src fp32 [2, rows, 64] of non-zero integers, mask fp32 (a ReLU pattern, every row positive somewhere),
      words int64 [2, rows] (the mask as bit words, built on the host), mask_rows int32 [rows] (a permutation) and
      words_rows (the words scattered so that words_rows[t][mask_rows[r]] = words[t][r]).

    With a slot map the entries marked dead in the layout name frames whose slot is -1; every live entry names a
    source row of its own."""
    lay = layout(name)
    n = lay.n
    rs = np.random.RandomState(1234 + seed)
    if use_slot:
        live = lay.live
        nl, nd = int(live.sum()), int((~live).sum())
        fl, fd = (nl + SUB - 1) // SUB + 1, (nd + SUB - 1) // SUB + 1
        frames = rs.permutation(fl + fd)
        slot = np.full(fl + fd, -1, dtype=np.int32)
        slot[frames[:fl]] = np.arange(fl - 1, -1, -1, dtype=np.int32)
        ids_l = (frames[:fl, None] * SUB + np.arange(SUB)[None]).reshape(-1)
        ids_d = (frames[fl:, None] * SUB + np.arange(SUB)[None]).reshape(-1)
        idx = np.empty(n, dtype=np.int64)
        idx[live] = ids_l[rs.permutation(len(ids_l))[:nl]]
        idx[~live] = ids_d[rs.permutation(len(ids_d))[:nd]]
        rows, sub = fl * SUB, SUB
        slot_t = torch.from_numpy(slot).to(device)
    else:
        live = np.ones(n, dtype=bool)
        rows, sub, slot_t = n + 3, 1, None
        idx = rs.permutation(rows)[:n].astype(np.int64)
    src = nonzero_ints((2, rows, 64), 11 + seed, 3, device)
    mask = relu_pattern((2, rows, 64), 12 + seed, device)
    words = words_of(mask).to(device)
    mrow = torch.from_numpy(rs.permutation(rows).astype(np.int32)).to(device)
    words_rows = torch.empty_like(words)
    words_rows[:, mrow.long()] = words
    # the conditions of the exact-integer rule
    counts = np.bincount(lay.keys[live], minlength=lay.nkeys) if live.any() else np.zeros(lay.nkeys)
    assert float(counts.max()) * 3 < LIMIT
    assert bool(((mask > 0) & (src != 0)).any(2).all())  # every source row shows, masked or not
    assert not torch.equal(src[0], src[1])
    return SimpleNamespace(lay=lay, keys=lay.keys, idx=idx, slot=slot_t, sub=sub, nkeys=lay.nkeys, L=lay.L, src=src,
                           mask=mask, words=words, mask_rows=mrow, words_rows=words_rows, live_entries=live)
