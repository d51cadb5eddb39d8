"""The task heads on the MI355X (csrc/gnx_heads.hip: gnx_node_ce, gnx_node_ce_backward, gnx_node_argmax, gnx_edge_scores,
gnx_edge_scores_backward) at their edges, against float64 numpy fed the float32 inputs widened to float64.  The raw entries are called
through gnntf._native: the pitches (ldl, ldf, ldg), the per-item losses and the accumulate contract are visible only there.

Criteria, none of them fitted to a kernel:
  * a loss item: |got - want| <= 1e-5 max(|want|, 1), the project's per-value tolerance; want = +inf has to be met exactly;
  * the mean: against the float64 mean of the kernel's OWN float32 items (the reduction alone), bound (D + 1) u mean |v| with D counted
    from the fixed tree (mean_roundings below), u = 2^-24;
  * a gradient element, summed by atomics in no fixed order: |got - want| <= 1e-4 |want| + (k + 4) u sum_i |term_i| over the k terms that
    hit the element -- the bound of a float32 sum of k terms in ANY order, plus the terms' own few roundings;
  * a link logit: 1e-4 |want| + (C + 4) u sum_c |F[u, c] F[v, c] r[c]|, the same bound for a dot product;
  * argmax: exact.
Operands that are column slices of a wider tensor sit in NaN: one read outside the slice poisons the result.  Buffers the kernels write
carry a sentinel wherever the header says nothing is written."""
import numpy as np
import pytest
import torch

from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                       # unit roundoff of float32
SENTINEL = -7.25
N_ROWS = 1000
PITCHES = ("dense", "odd", "quad")
OFFSETS = {"offset_1e3": 1e3, "offset_1e4": 1e4, "offset_-1e4": -1e4, "offset_1e6": 1e6}
REGIMES = ("plain",) + tuple(OFFSETS) + ("spread", "equal", "neginf", "label_neginf")


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def f64(x):
    return np.asarray(x, dtype=np.float64)


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def untouched(t, value):
    """Every element of ``t`` still holds ``value``, bit for bit."""
    return bool(torch.equal(t, torch.full_like(t, value)))


def place(x, pitch):
    """``x`` [n, C] on the device: as it is, or as the column slice of a wider tensor of NaNs --
    "odd": columns 1 .. C of [n, C + 3]: ld = C + 3 and a base 4 bytes past a row's start, so not 16-byte aligned;
    "quad": columns 4 .. C + 3 of a tensor whose width is a multiple of 4: ld % 4 == 0 and ld > C."""
    if pitch == "dense":
        return dev(x)
    n, C = x.shape
    left, ld = (1, C + 3) if pitch == "odd" else (4, (C + 11) // 4 * 4)
    view = filled((n, ld), float("nan"))[:, left:left + C]
    view.copy_(dev(x))
    assert view.stride(0) == ld > C and view.data_ptr() % 16 == (4 if pitch == "odd" else 0)
    return view


def assert_items(what, got, want):
    """Every item: +inf exactly, the others within the project's per-value tolerance."""
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), what
    ratio = float((np.abs(got[fin] - want[fin]) / (1e-5 * np.maximum(np.abs(want[fin]), 1.0))).max()) if fin.any() else 0.0
    print(f"{what}: worst item error / tolerance = {ratio:.4g}")
    assert ratio <= 1.0, f"{what}: worst item error / tolerance = {ratio:.4g}"


def assert_within(what, got, want, bound):
    """|got - want| <= bound per element; where the bound is 0 (nothing may have been added) the value is exact."""
    err = np.abs(f64(got) - want)
    exact = bound == 0
    assert (err[exact] == 0).all(), f"{what}: an element that no item names was written"
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.4g}")
    assert ratio <= 1.0, f"{what}: worst error / bound = {ratio:.4g}"


# ---- node loss, forward --------------------------------------------------------------------------------------------------------------
def node_case(regime, seed, n, C, m):
    """(logits float32 [n, C], nodes [m] with repeats, labels [m]) of one logit regime."""
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((n, C))
    nodes = rng.integers(0, n, size=m)
    if m >= 2:
        nodes[-1] = nodes[0]                                             # a repeat at every m
    labels = rng.integers(0, C, size=m)
    if regime in OFFSETS:
        x += OFFSETS[regime]
    elif regime == "spread":                                             # one column 1e4 above the rest: every other exponential underflows
        top = rng.integers(0, C, size=n)
        x[np.arange(n), top] += 1e4
        labels = np.where(np.arange(m) % 2 == 0, top[nodes], (top[nodes] + 1) % C)      # on the maximum (want ~ 0) and off it
    elif regime == "equal":
        x[:] = x[:, :1]
    elif regime == "neginf":                                             # -inf in columns that are no item's label; never a whole row
        hole = rng.random((n, C)) < 0.4
        hole[np.arange(n), rng.integers(0, C, size=n)] = False
        x[hole] = -np.inf
        labels = (rng.random((m, C)) * ~hole[nodes]).argmax(axis=1)      # uniform over the finite columns of the item's row
        assert np.isfinite(x[nodes, labels]).all()
    elif regime == "label_neginf":                                       # the label's own column is -inf: the loss is +inf
        assert C >= 2
        for i in {0, m // 2, m - 1}:
            if np.isfinite(x[nodes[i]]).all():
                x[nodes[i], labels[i]] = -np.inf
    else:
        assert regime == "plain"
    return x.astype(np.float32), nodes, labels


def loss_items64(x, nodes, labels):
    """logsumexp(x) - x[label] in float64 (as -log_softmax: the maximum is taken out first, so an offset costs nothing)."""
    return -orc.log_softmax(f64(x)[nodes])[np.arange(len(nodes)), labels]


def mean_roundings(m):
    """D of gnx_node_ce's mean: the float32 roundings on the longest path from an item to d_mean_loss, read off k_mean_partial / k_mean.
    block256_sum over ``count`` values: a thread adds its ceil(count / 256) values one by one, the first into an exact zero, so
    ceil(count / 256) - 1 roundings; then the LDS tree of 256 slots, 8 levels, 8 roundings.  m <= 4096: one block over all m items and the
    division, D = ceil(m / 256) - 1 + 8 + 1.  m > 4096: 256 blocks over slices of per = ceil(m / 256) items, one block over the 256
    partial sums (ceil(256 / 256) - 1 = 0, then 8), and the division: D = (ceil(per / 256) - 1 + 8) + 8 + 1.  (float)m is exact below
    2^24.  A sum of this shape is off by at most gamma_D sum |v| <= (D + 1) u sum |v| for D u << 1; divided by m that is the bound."""
    def block(count):
        return -(-count // 256) - 1 + 8
    return (block(-(-m // 256)) + block(256) if m > 4096 else block(m)) + 1


def assert_mean(what, items, mean, m):
    v = f64(items)
    if not np.isfinite(v).all():
        assert mean == v.mean(), what                                    # +inf items: the mean is +inf
        return
    D = mean_roundings(m)
    err, bound = abs(float(mean) - v.mean()), (D + 1) * U * np.abs(v).mean()
    print(f"{what}: D = {D}, mean error {err:.3g}, bound {bound:.3g}")
    assert err <= bound, f"{what}: D = {D}, mean error {err:.3g}, bound {bound:.3g}"


def raw_node_ce(gnntf, L, nodes, labels, tail=300):
    """gnx_node_ce itself: (items [m], mean) as float32 numpy.  d_loss_per_node is allocated ``tail`` floats longer than the m + 256 the
    header asks for; those must come back as they went in."""
    nat = gnntf._native
    m = nodes.numel()
    per_item, mean = filled((m + 256 + tail,), SENTINEL), filled((1,), SENTINEL)
    nat.check(nat.lib().gnx_node_ce(nat.ptr(L), L.stride(0), L.shape[0], L.shape[1], nat.ptr(nodes), nat.ptr(labels), m, nat.ptr(per_item),
                                    nat.ptr(mean), nat.current_stream()))
    assert untouched(per_item[m + 256:], SENTINEL), "gnx_node_ce wrote past the m + 256 floats of d_loss_per_node"
    return host(per_item[:m]), host(mean)[0]


# m: the group of 16 items, the block of 256, the one-level mean's last m (4096) and the two-level mean's first (4097).  At m = 4097 a
# slice has ceil(4097 / 256) = 17 items and 256 * 17 - 4097 = 255 >= 17: blocks 241 .. 255 get an EMPTY slice (block 241 starts at
# 4097 = m, the later ones past it).  At m = 4352 = 256 * 17 and m = 65536 = 256 * 256 the slices end exactly at m; at m = 65537 the
# last block holds 2 items.
M_AND_C = ((1, 1), (1, 40), (15, 2), (16, 15), (17, 16), (255, 17), (256, 40), (4095, 129), (4096, 40), (4097, 17), (4097, 129), (4352, 16),
           (65536, 2), (65537, 40))


@pytest.mark.parametrize("m,C", M_AND_C)
def test_node_ce_item_counts(gnntf, m, C):
    x, nodes, labels = node_case("plain", 100 * C + m, N_ROWS, C, m)
    items, mean = raw_node_ce(gnntf, dev(x), dev(nodes), dev(labels))
    assert_items(f"m = {m}, C = {C}", items, loss_items64(x, nodes, labels))
    assert_mean(f"m = {m}, C = {C}", items, mean, m)


@pytest.mark.parametrize("regime", REGIMES)
def test_node_ce_regimes(gnntf, regime):
    """2000 items at C = 2, 17, 40 and 129 per logit regime.  On the loss form (log(se) + mx) - x[label] the offset regimes fail: log(se)
    is rounded to the spacing of mx before the offset cancels (worst item error 5e-4 at an offset of 1e4, 3e-2 at 1e6)."""
    for C in (2, 17, 40, 129):
        x, nodes, labels = node_case(regime, 7 * C, 700, C, 2000)
        want = loss_items64(x, nodes, labels)
        if regime == "label_neginf":
            assert np.isposinf(want).any()
        if regime == "spread":
            assert (want[0::2] < 1e-300).all() and (want[1::2] > 9e3).all()
        items, mean = raw_node_ce(gnntf, dev(x), dev(nodes), dev(labels))
        assert_items(f"{regime}, C = {C}", items, want)
        assert_mean(f"{regime}, C = {C}", items, mean, 2000)


@pytest.mark.parametrize("pitch", PITCHES[1:])
@pytest.mark.parametrize("C", (1, 2, 15, 16, 17, 40, 129))
def test_node_ce_pitched_logits(gnntf, C, pitch):
    """A column slice of a wider tensor reaches the kernels as it is (no copy), through gnntf.node_ce and through the raw entry."""
    m = 333
    x, nodes, labels = node_case("plain", C, N_ROWS, C, m)
    want = loss_items64(x, nodes, labels)
    L = place(x, pitch)
    assert gnntf.sparse._as_f32_rows(L).data_ptr() == L.data_ptr()
    items, mean = raw_node_ce(gnntf, L, dev(nodes), dev(labels))
    assert_items(f"{pitch}, C = {C}", items, want)
    assert_mean(f"{pitch}, C = {C}", items, mean, m)
    loss = gnntf.node_ce(L.requires_grad_(), dev(nodes), dev(labels))
    assert host(loss).view(np.int32) == mean.view(np.int32)             # the same call, so the same bits
    (loss * 1.7).backward()
    ref, bound = node_grad_ref(x, nodes, labels, np.float32(1.7))
    assert_within(f"gnntf.node_ce backward, {pitch}, C = {C}", host(L.grad), ref, bound)


def test_node_ce_is_reproducible(gnntf):
    """The fixed reduction order: two calls, the same bits, at the largest m (two-level mean)."""
    x, nodes, labels = node_case("plain", 5, N_ROWS, 40, 65537)
    L, nd, lb = dev(x), dev(nodes), dev(labels)
    (a, mean_a), (b, mean_b) = raw_node_ce(gnntf, L, nd, lb), raw_node_ce(gnntf, L, nd, lb)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and mean_a.view(np.int32) == mean_b.view(np.int32)


# ---- node loss, backward -------------------------------------------------------------------------------------------------------------
def node_grad_ref(x, nodes, labels, g, prefill=None):
    """(want, bound) of d_grad_logits [n, C] in float64: g / m (softmax - onehot) added per node over the items in range, m counting
    every item; bound = 1e-4 |want| + (k + 4) u sum |term|, a pre-filled value being one more term."""
    n, C = x.shape
    ok = (nodes >= 0) & (nodes < n) & (labels >= 0) & (labels < C)
    nd, lb = nodes[ok], labels[ok]
    terms = np.exp(orc.log_softmax(f64(x)[nd]))
    terms[np.arange(len(nd)), lb] -= 1.0
    terms *= float(g) / len(nodes)
    want, mag = np.zeros((n, C)), np.zeros((n, C))
    np.add.at(want, nd, terms)
    np.add.at(mag, nd, np.abs(terms))
    k = f64(np.bincount(nd, minlength=n))[:, None]
    if prefill is not None:
        want, mag, k = want + f64(prefill), mag + np.abs(f64(prefill)), k + 1
    return want, 1e-4 * np.abs(want) + (k + 4) * U * mag


def raw_node_ce_backward(gnntf, L, nodes, labels, g, pad=0, prefill=None):
    """gnx_node_ce_backward into d_grad_logits [n, C + pad]: zeros (or ``prefill``) in the C columns, the sentinel in the padding, which
    must keep it bit for bit.  Returns the C columns."""
    nat = gnntf._native
    n, C = L.shape
    grad = filled((n, C + pad), SENTINEL)
    grad[:, :C] = 0.0 if prefill is None else dev(prefill)
    gd = dev(np.array([g], dtype=np.float32))
    nat.check(nat.lib().gnx_node_ce_backward(nat.ptr(L), L.stride(0), n, C, nat.ptr(nodes), nat.ptr(labels), nodes.numel(), nat.ptr(gd),
                                             nat.ptr(grad), grad.stride(0), nat.current_stream()))
    assert untouched(grad[:, C:], SENTINEL), "gnx_node_ce_backward wrote into the padding columns of d_grad_logits"
    return host(grad[:, :C])


@pytest.mark.parametrize("regime", REGIMES)
def test_node_ce_backward_regimes(gnntf, regime):
    """The forward regimes, at a gradient pitch of C + 5 and d_grad_loss = 1.7.  n = 700 rows, 500 items: rows that no item names stay
    exactly zero (their bound is 0).  Formed as softmax - 1, the label's column misses the bound at C = 2 in every regime with drawn
    logits (error / bound 1.4 "plain" to 4.9 "offset_1e4"; 39 at the 333 items of test_node_ce_pitched_logits): where the model is sure
    of the label the term is 1e-3 or less and keeps only the absolute 1e-7 of the softmax."""
    for C in (2, 17, 40, 129):
        x, nodes, labels = node_case(regime, 11 * C, 700, C, 500)
        got = raw_node_ce_backward(gnntf, dev(x), dev(nodes), dev(labels), 1.7, pad=5)
        want, bound = node_grad_ref(x, nodes, labels, np.float32(1.7))
        assert (bound == 0).all(axis=1).sum() >= 700 - 500
        assert_within(f"{regime}, C = {C}", got, want, bound)


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("C", (1, 15, 16, 17, 129))
def test_node_ce_backward_accumulates(gnntf, C, pitch):
    """+= into what the caller left there, a negative d_grad_loss, pitched logits and a pitched gradient."""
    m = 257
    x, nodes, labels = node_case("plain", 3 * C, N_ROWS, C, m)
    prefill = np.random.default_rng(C).standard_normal(x.shape).astype(np.float32)
    got = raw_node_ce_backward(gnntf, place(x, pitch), dev(nodes), dev(labels), -0.6, pad=5, prefill=prefill)
    want, bound = node_grad_ref(x, nodes, labels, np.float32(-0.6), prefill)
    assert_within(f"pre-filled, {pitch}, C = {C}", got, want, bound)
    named = np.zeros(len(x), dtype=bool)
    named[nodes] = True
    assert np.array_equal(got[~named].view(np.int32), prefill[~named].view(np.int32))        # rows that no item names: not a bit moved
    got = raw_node_ce_backward(gnntf, place(x, pitch), dev(nodes), dev(labels), -0.6)       # ldg == C
    want, bound = node_grad_ref(x, nodes, labels, np.float32(-0.6))
    assert_within(f"zero-filled, {pitch}, C = {C}", got, want, bound)


@pytest.mark.parametrize("C", (2, 17, 40))
def test_node_ce_backward_contention(gnntf, C):
    """4097 items, labels over all classes, all on ONE node; then on two nodes in turn.  Each element takes 4097 (2049, 2048) atomics."""
    m = 4097
    x, _, labels = node_case("plain", C, 50, C, m)
    assert len(np.unique(labels)) == C
    for what, nodes in (("one node", np.full(m, 31)), ("two nodes", np.where(np.arange(m) % 2 == 0, 7, 8))):
        got = raw_node_ce_backward(gnntf, dev(x), dev(nodes), dev(labels), 1.7, pad=5)
        want, bound = node_grad_ref(x, nodes, labels, np.float32(1.7))
        assert_within(f"{what}, C = {C}", got, want, bound)


def test_node_ce_backward_skips_items_out_of_range(gnntf):
    """A node id == n_rows and a label == C among good items (device tensors: no host check).  Those two give no gradient -- the row the
    bad label's item names stays zero -- and the scale of the others is still g / m with m counting all items."""
    n, C, m = 300, 17, 40
    x, nodes, labels = node_case("plain", 1, n, C, m)
    nodes[:] = np.arange(m) * 3                                          # distinct: row nodes[20] is named by the bad label's item alone
    nodes[9], labels[20] = n, C
    got = raw_node_ce_backward(gnntf, dev(x), dev(nodes), dev(labels), 1.7, pad=5)
    want, bound = node_grad_ref(x, nodes, labels, np.float32(1.7))
    assert (want[nodes[20]] == 0).all() and (bound[nodes[20]] == 0).all() and np.count_nonzero(want.any(axis=1)) == m - 2
    assert_within("items out of range", got, want, bound)
    items, mean = raw_node_ce(gnntf, dev(x), dev(nodes), dev(labels))
    good = np.ones(m, dtype=bool)
    good[[9, 20]] = False
    assert np.isnan(items[~good]).all() and np.isnan(mean)
    assert_items("the items in range", items[good], loss_items64(x, nodes[good], labels[good]))


# ---- argmax --------------------------------------------------------------------------------------------------------------------------
def raw_argmax(gnntf, L, nodes=None):
    nat = gnntf._native
    m = L.shape[0] if nodes is None else nodes.numel()
    out = filled((m + 8,), -77, torch.int64)
    nat.check(nat.lib().gnx_node_argmax(nat.ptr(L), L.stride(0), L.shape[0], L.shape[1], nat.ptr(nodes), m, nat.ptr(out), nat.current_stream()))
    assert untouched(out[m:], -77)
    return host(out[:m])


def argmax_everywhere(gnntf, what, rows, want):
    """``rows`` through both paths (all rows / listed rows with repeats), every pitch, the raw entry and gnntf.node_argmax."""
    listed = np.concatenate([np.arange(len(rows))[::-1], np.arange(len(rows))[::2]])
    for pitch in PITCHES:
        L = place(rows, pitch)
        assert gnntf.sparse._as_f32_rows(L).data_ptr() == L.data_ptr()
        for got in (raw_argmax(gnntf, L), host(gnntf.node_argmax(L))):
            assert np.array_equal(got, want), (what, pitch, np.flatnonzero(got != want)[:8])
        for got in (raw_argmax(gnntf, L, dev(listed)), host(gnntf.node_argmax(L, dev(listed)))):
            assert np.array_equal(got, want[listed]), (what, pitch, "listed", np.flatnonzero(got != want[listed])[:8])


def tie_rows(C):
    """Hand-made rows over a base without ties (-1, -2, ...: its own maximum is column 0) and the index each must give."""
    rows, want = [], []

    def add(index, *cells):
        rows.append(planted(C, *cells))
        want.append(index)

    everywhere = tuple(range(C))
    add(C - 1, ((C - 1,), 5.0))                                         # the maximum in the last column only
    add(0, ((0, C - 1), 5.0))                                           # the first and the last column
    add(0, ((0, C - 1), np.inf))                                        # +inf twice
    if C >= 3:
        add(1, ((1, C - 1), np.inf))
        add(C - 2, ((C - 2, C - 1), 5.0))                               # neighbouring lanes
    if C > 16:
        for c in {0, C - 17}:
            add(c, ((c, c + 16), 5.0))                                  # columns c and c + 16: the same lane's next column
    if C > 17:
        add(2, ((2, 17), 5.0))                                          # lane 1's higher column against lane 2's lower one
        add(1, ((1, 16, 17), 5.0))
    add(0, ((C - 1,), 0.0), ((0,), -0.0))                               # -0.0 before +0.0: they compare equal, the first wins
    add(0, (everywhere, 2.5))                                           # all equal
    add(0, (everywhere, -np.inf))                                       # all -inf
    return np.stack(rows), np.array(want)


def planted(C, *cells):
    """The base row -1, -2, ..., -C (no ties, its maximum in column 0) with ``value`` written into ``columns`` for each (columns, value)."""
    row = -(1.0 + np.arange(C, dtype=np.float32))
    for columns, value in cells:
        row[list(columns)] = value
    return row


def nan_rows(C):
    """Rows holding NaNs.  A NaN never wins: the first index of the maximum over the other entries; a row of only NaNs gives 0."""
    nan, everywhere = np.float32("nan"), tuple(range(C))
    rows = [planted(C, (everywhere, nan))]
    if C >= 2:
        rows += [planted(C, ((0,), nan)), planted(C, ((C - 1,), nan)), planted(C, ((0,), nan), ((C - 1,), 5.0)),
                 planted(C, ((0,), 5.0), ((C - 1,), nan)), planted(C, (everywhere, nan), ((C - 1,), -3.0))]
    if C >= 3:                                                           # a NaN before, between and after two maxima
        rows += [planted(C, ((0,), nan), ((1, C - 1), 5.0)), planted(C, ((1,), nan), ((0, C - 1), 5.0)), planted(C, ((C - 1,), nan), ((0, 1), 5.0))]
    if C > 17:                                                           # ... and within one lane's columns (1 and 17; 0, 16 and 32)
        rows += [planted(C, ((1,), nan), ((17,), 5.0)), planted(C, ((17,), nan), ((1,), 5.0)), planted(C, ((1,), nan), ((17, 18), 5.0)),
                 planted(C, ((0, 16, 32 % C), nan))]
    rows = np.stack(rows)
    others = np.where(np.isnan(rows), -np.inf, rows)
    assert (np.isfinite(others).any(axis=1) | np.isnan(rows).all(axis=1)).all()      # no row mixes only NaN and -inf
    return rows, others.argmax(axis=1)


@pytest.mark.parametrize("C", (1, 2, 15, 16, 17, 32, 33, 129))
def test_argmax_ties_and_specials(gnntf, C):
    rows, want = tie_rows(C)
    assert np.array_equal(rows.argmax(axis=1), want)                     # np.argmax on the same float32 rows agrees with the hand
    argmax_everywhere(gnntf, f"ties, C = {C}", rows, want)
    rows, want = nan_rows(C)
    argmax_everywhere(gnntf, f"NaNs, C = {C}", rows, want)
    rng = np.random.default_rng(C)
    rows = (3.0 * rng.standard_normal((700, C))).astype(np.float32)
    argmax_everywhere(gnntf, f"drawn, C = {C}", rows, rows.argmax(axis=1))


def test_argmax_many_ties(gnntf):
    """2000 rows of integers in [-3, 3] at C = 33: several maxima in almost every row."""
    rows = np.random.default_rng(33).integers(-3, 4, size=(2000, 33)).astype(np.float32)
    assert ((rows == rows.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.9
    argmax_everywhere(gnntf, "integers", rows, rows.argmax(axis=1))


# ---- link head -----------------------------------------------------------------------------------------------------------------------
def in_range(edges, n):
    return ((edges >= 0) & (edges < n)).all(axis=1)


def edge_ref(F, edges, r):
    """(want, bound) of the logits in float64; NaN for an edge with an endpoint out of range."""
    n, C = F.shape
    ok = in_range(edges, n)
    e = edges[ok]
    want, mag = np.full(len(edges), np.nan), np.zeros(len(edges))
    want[ok] = orc.link_logits(f64(F), e, None if r is None else f64(r)[:, None])
    mag[ok] = np.abs(f64(F)[e[:, 0]] * f64(F)[e[:, 1]] * (1.0 if r is None else f64(r))).sum(axis=1)
    return want, 1e-4 * np.abs(want) + (C + 4) * U * mag


def edge_grad_ref(F, edges, r, g, prefill=None):
    """(want, bound) of d_grad_F: dF[u] += g r F[v] and dF[v] += g r F[u] over the edges in range, in float64."""
    n, C = F.shape
    ok = in_range(edges, n)
    u, v = edges[ok, 0], edges[ok, 1]
    w = f64(g)[ok, None] * (1.0 if r is None else f64(r))
    want, mag = np.zeros((n, C)), np.zeros((n, C))
    for rows, terms in ((u, w * f64(F)[v]), (v, w * f64(F)[u])):
        np.add.at(want, rows, terms)
        np.add.at(mag, rows, np.abs(terms))
    k = f64(np.bincount(u, minlength=n) + np.bincount(v, minlength=n))[:, None]
    if prefill is not None:
        want, mag, k = want + f64(prefill), mag + np.abs(f64(prefill)), k + 1
    return want, 1e-4 * np.abs(want) + (k + 4) * U * mag


def raw_edge_scores(gnntf, F, edges, r):
    nat = gnntf._native
    m = edges.shape[0]
    out = filled((m + 8,), SENTINEL)
    nat.check(nat.lib().gnx_edge_scores(nat.ptr(F), F.stride(0), F.shape[0], F.shape[1], nat.ptr(edges), m, nat.ptr(r), nat.ptr(out),
                                        nat.current_stream()))
    assert untouched(out[m:], SENTINEL)
    return host(out[:m])


def raw_edge_scores_backward(gnntf, F, edges, r, g, pad=0, prefill=None):
    nat = gnntf._native
    n, C = F.shape
    grad = filled((n, C + pad), SENTINEL)
    grad[:, :C] = 0.0 if prefill is None else dev(prefill)
    nat.check(nat.lib().gnx_edge_scores_backward(nat.ptr(F), F.stride(0), n, C, nat.ptr(edges), edges.shape[0], nat.ptr(r), nat.ptr(g),
                                                 nat.ptr(grad), grad.stride(0), nat.current_stream()))
    assert untouched(grad[:, C:], SENTINEL), "gnx_edge_scores_backward wrote into the padding columns of d_grad_F"
    return host(grad[:, :C])


def assert_scores(what, got, want, bound):
    bad = np.isnan(want)
    assert np.array_equal(np.isnan(got), bad), f"{what}: NaN at other edges than those out of range"
    assert_within(what, got[~bad], want[~bad], bound[~bad])


def link_operands(C, n=N_ROWS):
    rng = np.random.default_rng(1000 + C)
    return rng.standard_normal((n, C)).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32), rng


@pytest.mark.parametrize("C", (1, 15, 16, 17, 40, 128))
def test_edge_scores_forward_and_backward(gnntf, C):
    """m = 0, 1, round the group of 16, and 5000 drawn edges; with and without the DistMult weights; every pitch of F; a gradient pitch of
    C + 5, into zeros and into a pre-filled d_grad_F."""
    F, r, rng = link_operands(C)
    prefill = rng.standard_normal(F.shape).astype(np.float32)
    for m in (0, 1, 15, 16, 17, 5000):
        edges = rng.integers(0, len(F), size=(m, 2))
        g = rng.standard_normal(m).astype(np.float32)
        for weights in (None, r):
            want, bound = edge_ref(F, edges, weights)
            for pitch in PITCHES if m in (17, 5000) else PITCHES[:1]:
                Fd, rd = place(F, pitch), None if weights is None else dev(weights)
                assert_scores(f"C = {C}, m = {m}, {pitch}", raw_edge_scores(gnntf, Fd, dev(edges), rd), want, bound)
                assert gnntf.sparse._as_f32_rows(Fd).data_ptr() == Fd.data_ptr()
                z = gnntf.edge_scores(Fd, dev(edges), None if weights is None else rd.reshape(C, 1))
                assert z.shape == (m,)
                assert_scores(f"gnntf.edge_scores, C = {C}, m = {m}, {pitch}", host(z), want, bound)
                got = raw_edge_scores_backward(gnntf, Fd, dev(edges), rd, dev(g), pad=5)
                assert_within(f"backward, C = {C}, m = {m}, {pitch}", got, *edge_grad_ref(F, edges, weights, g))
            got = raw_edge_scores_backward(gnntf, dev(F), dev(edges), None if weights is None else dev(weights), dev(g), pad=5, prefill=prefill)
            if m == 0:
                assert np.array_equal(got.view(np.int32), prefill.view(np.int32))
            assert_within(f"backward, pre-filled, C = {C}, m = {m}", got, *edge_grad_ref(F, edges, weights, g, prefill))


def test_edge_scores_of_no_edges(gnntf):
    """m = 0: an empty result through gnntf.edge_scores for a [0, 2] int64 device tensor; the raw entry is OK and leaves d_out alone."""
    F = dev(link_operands(16)[0])
    none = dev(np.empty((0, 2), dtype=np.int64))
    z = gnntf.edge_scores(F, none)
    assert z.shape == (0,) and z.dtype == torch.float32 and z.device == F.device
    assert raw_edge_scores(gnntf, F, none, None).shape == (0,)          # (its 8 floats of d_out keep the sentinel)


@pytest.mark.parametrize("C", (1, 17, 40))
def test_edge_scores_backward_contention(gnntf, C):
    """Self-loops only (u == v: one thread's two atomics land on one address, dF[u] = 2 g r F[u] over the loops), one edge 1000 times, and a
    star of 4097 edges that all share endpoint 0, on either side."""
    F, r, rng = link_operands(C, n=200)
    loops = np.repeat(rng.integers(0, 200, size=(500, 1)) % 37, 2, axis=1)
    spokes = rng.integers(0, 200, size=4097)
    star = np.where((np.arange(4097) % 2 == 0)[:, None], np.stack([np.zeros(4097, dtype=np.int64), spokes], 1), np.stack([spokes, np.zeros(4097, dtype=np.int64)], 1))
    for what, edges in (("self-loops", loops), ("one edge 1000 times", np.tile(np.array([[5, 9]]), (1000, 1))), ("star", star)):
        g = rng.standard_normal(len(edges)).astype(np.float32)
        for weights in (None, r):
            rd = None if weights is None else dev(weights)
            assert_scores(f"{what}, C = {C}", raw_edge_scores(gnntf, dev(F), dev(edges), rd), *edge_ref(F, edges, weights))
            got = raw_edge_scores_backward(gnntf, dev(F), dev(edges), rd, dev(g), pad=5)
            want, bound = edge_grad_ref(F, edges, weights, g)
            assert_within(f"backward, {what}, C = {C}", got, want, bound)
            if what == "self-loops":                                     # the closed form of the docstring, so the reference is checked too
                twice = np.zeros_like(want)
                np.add.at(twice, edges[:, 0], 2.0 * f64(g)[:, None] * f64(F)[edges[:, 0]] * (1.0 if weights is None else f64(weights)))
                np.testing.assert_allclose(want, twice, rtol=1e-12, atol=1e-300)


def test_edge_scores_out_of_range(gnntf):
    """A negative endpoint and an endpoint == n_rows among good edges (device tensors: no host check): NaN at exactly those two, and the
    gradient of the good edges alone."""
    C = 17
    F, r, rng = link_operands(C, n=300)
    edges = rng.integers(0, 300, size=(60, 2))
    edges[7], edges[33] = (-1, 3), (5, 300)
    g = rng.standard_normal(60).astype(np.float32)
    want, bound = edge_ref(F, edges, r)
    assert np.flatnonzero(np.isnan(want)).tolist() == [7, 33]
    assert_scores("forward", raw_edge_scores(gnntf, dev(F), dev(edges), dev(r)), want, bound)
    assert_scores("gnntf.edge_scores", host(gnntf.edge_scores(dev(F), dev(edges), dev(r).reshape(C, 1))), want, bound)
    got = raw_edge_scores_backward(gnntf, dev(F), dev(edges), dev(r), dev(g), pad=5)
    assert_within("backward", got, *edge_grad_ref(F, edges, r, g))
