"""The batch-norm kernels (csrc/bn/batchnorm.hip) at every edge of their work
split, through the split-phase entry points and against the fp64 references of
tests/exact_ref.py.

Two kinds of input, each with a bound that needs no measurement:
  * exact cases.  x, dy and the residual are integers in [-3, 3], so the fp32
    partials and the fp64 reduce of the moments kernels are exact.  The apply
    kernels take their moments as an input, so the moments are crafted: a
    power-of-two count, an integer mean, a variance of exactly 1/4 and eps = 0
    give invstd = 2; with weights in {+-0.5, +-1, 2} and integer biases every
    coefficient, output and gradient is a small multiple of 1/4 that fp32 and
    bf16 hold.  The kernel must then equal the reference bit for bit: a
    dropped row, lane, chunk or zeroing shows in plain sight.
  * randn data with per-channel offsets of 0, 4 and 16 standard deviations,
    under bounds from fp32 fused-multiply-add arithmetic alone (U = 2^-24):
      moments   |sum - ref| <= n*U*sum|x|, |sumsq - ref| <= (n+1)*U*sum x^2,
                n = rows_per_block, the longest fp32 chain;
      apply     |y - ref| <= 8*U*(|x*sc| + |mean*sc| + |b| + |res|) (+ 2^-8*|ref|
                for a bf16 output), ref being fed the kernel's own moments;
      backward  the same on |a*dz| + |b*x| + |c|.
A case that exists to reach a branch reads the host's own work split
(``bn_plan``) and asserts that the branch is still reached; the shapes live in
tests/bn_edge_shapes.py, which tests/test_bn_plan_cpu.py checks without a GPU."""
import pytest
import torch

from distributed_model_parallel_amd import _native
from tests import bn_edge_shapes as S
from tests import exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
INF = float("inf")
COUNT = 64.0  # the crafted moments' row count: a power of two, not M


def _ints(shape, dtype, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, device=DEV, dtype=torch.int8).to(dtype)


def _exact(out, ref, what):
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    torch.testing.assert_close(out.double(), ref.double(), atol=0, rtol=0, msg=lambda m: f"{what}: {m}")


def _stored(ref, dtype, what):
    """The reference survives a round trip through the dtype the kernel stores."""
    assert bool((ref.float().to(dtype).double() == ref).all()), f"{what}: {dtype} does not hold the reference"
    return ref


def _partials_fit(largest_term, g, what):
    """Every fp32 partial of a block (at most rows_per_block terms per channel) stays an exact integer."""
    assert float(largest_term) * g["rows_per_block"] < 2 ** 24, what


def _within(out, ref, bound, what):
    err = (out.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err/bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: err/bound = {worst:.3f}"


def _half_ulp(ref, dtype):
    return R.BF16_HALF_ULP * ref.abs() if dtype == BF16 else torch.zeros_like(ref)


class Crafted:
    """Per-channel parameters and moments that make every BN coefficient dyadic."""

    def __init__(self, c, weight=True, bias=True):
        self.c = c
        self.w = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0], device=DEV)[torch.randint(0, 5, (c,), device=DEV)] \
            if weight else None
        self.b = _ints((c,), F32, -2, 2) if bias else None
        self.mean = _ints((c,), F32, -2, 2)
        self.invstd = torch.full((c,), 2.0, device=DEV)
        m = self.mean.double()
        self.sums = torch.cat([COUNT * m, COUNT * (m * m + 0.25), m.new_tensor([COUNT])])
        self.rm0 = _ints((c,), F32, -4, 4)
        self.rv0 = _ints((c,), F32, 1, 8) / 4
        # backward: a = w*2, b = -a*k/4, c = -a*j/4 - b*mean with sdz = 16 j, sdzx = 4 k
        self.bsums = torch.cat([16.0 * _ints((c,), F64, -2, 2), 4.0 * _ints((c,), F64, -2, 2)])
        self.count = torch.tensor([COUNT], dtype=F64, device=DEV)
        self.coef = R.bn_fwd_coeffs(self.sums, self.w, self.b, 0.0)
        assert bool((self.coef[2] == 2.0).all()) and bool((self.coef[0] == m).all())

    @property
    def scale(self):
        return self.coef[3]

    @property
    def shift(self):
        return self.coef[4]


def _running_ok(rm, rv, cr, what):
    """momentum 0.5: the mean update is exact; the variance update holds n/(n-1),
    compared with the fp64 expression rounded to fp32 within 2U relative (one
    rounding of the unbiased variance, one of a contracted multiply-add)."""
    mean, var = cr.coef[0], cr.coef[1]
    nrm, nrv = R.bn_running_update(cr.rm0, cr.rv0, mean, var.float().double(), COUNT, 0.5)
    _exact(rm, nrm, what + " running_mean")
    _within(rv, nrv.float().double(), 2 * R.U * nrv.abs(), what + " running_var")


def _forward_exact(C, x, cr, res, relu, clip, what, g):
    """bn_forward_apply on crafted moments, everything it returns or updates; returns the reference y."""
    c, dtype = cr.c, x.dtype
    rm, rv = cr.rm0.clone(), cr.rv0.clone()
    nbt = torch.tensor([41], device=DEV)
    y, sm, si = C.bn_forward_apply(x, cr.sums, cr.w, cr.b, rm, rv, 0.5, 0.0, res, relu, c, nbt, False, clip)
    yr = _stored(R.bn_apply(x, cr.scale, cr.shift, res, relu, clip), dtype, what)
    assert y.dtype == dtype
    _exact(y, yr, what + " y")
    _exact(sm, cr.coef[0], what + " save_mean")
    _exact(si, cr.coef[2], what + " save_invstd")
    _running_ok(rm, rv, cr, what)
    assert nbt.item() == 42, what
    if relu and res is None and dtype == BF16:  # the moments of the stored output, from the same pass
        _partials_fit(yr.abs().max() ** 2, g, what)
        y2, _, _, os_ = C.bn_forward_apply(x, cr.sums, cr.w, cr.b, None, None, 0.5, 0.0, None, True, c, None,
                                           True, clip)
        _exact(y2, yr, what + " y with out_moments")
        _exact(os_, R.bn_moments(yr), what + " output moments")
    return yr


def _backward_exact(C, dy, x, cr, mode, y, clip, g, what):
    """bn_backward_moments and every bn_backward_apply variant of one mask mode."""
    c, dtype = cr.c, x.dtype
    relu = mode != 0
    mask = None if mode == 0 else R.bn_mask_from_y(y, clip) if mode == 1 else \
        R.bn_mask_from_x(x, cr.scale, cr.shift, clip)
    yk = y.float().to(dtype) if mode == 1 else None
    sums = C.bn_backward_moments(dy, x, yk, cr.mean, relu, c, cr.w, cr.b, cr.invstd, clip)
    _partials_fit(15, g, what)  # |dz * (x - mean)| <= 3 * 5
    assert sums.dtype == F64
    _exact(sums, R.bn_bwd_moments(dy, x, cr.mean, mask), f"{what} backward moments mode {mode}")
    for training in (True, False):
        a, b, cc, dwr, dbr = R.bn_bwd_coeffs(cr.bsums, COUNT, cr.w, cr.mean, cr.invstd, training)
        dxr, dzr = R.bn_bwd_apply(dy, x, a, b, cc, mask)
        _stored(dxr, dtype, what)
        for want_dres in (False, True):
            w2 = f"{what} backward apply mode {mode} training {training} dres {want_dres}"
            dx, dw, db, dres = C.bn_backward_apply(dy, x, yk, cr.bsums, cr.count, cr.w, cr.mean, cr.invstd, training,
                                                   relu, want_dres, c, cr.b, clip)
            _exact(dx, dxr, w2 + " dx")
            _exact(dw, dwr, w2 + " dweight")
            _exact(db, dbr, w2 + " dbias")
            if want_dres:
                _exact(dres, dzr, w2 + " dres")
            else:
                assert dres is None
        # accumulation into gradients that already hold something
        pw, pb = _ints((c,), F32, 1, 5), _ints((c,), F32, -5, -1)
        aw, ab = pw.clone(), pb.clone()
        dx, dw, db, _ = C.bn_backward_apply(dy, x, yk, cr.bsums, cr.count, cr.w, cr.mean, cr.invstd, training, relu,
                                            False, c, cr.b, clip, aw, ab)
        assert dw is None and db is None
        _exact(dx, dxr, what + " acc dx")
        _exact(aw, dwr + pw.double(), what + " accumulated dweight")
        _exact(ab, dbr + pb.double(), what + " accumulated dbias")


def _battery(C, m, c, dtype, weight=True, bias=True):
    """Every kernel of the file on one integer [m, c] problem, all compared exactly."""
    g = C.bn_plan(m, c, dtype)
    what = f"M={m} C={c} {dtype} w={weight} b={bias}"
    x, dy, res = _ints((m, c), dtype), _ints((m, c), dtype), _ints((m, c), dtype)
    cr = Crafted(c, weight, bias)
    # moments
    _partials_fit(9, g, what)
    sums = C.bn_local_moments(x, c)
    assert sums.dtype == F64
    _exact(sums, R.bn_moments(x), what + " moments")
    # forward apply: each of {relu, residual}, ReLU and ReLU6
    ys = {}
    for relu, clip in ((False, INF), (True, INF), (True, 6.0)):
        for r in (None, res):
            ys[(clip, r is not None)] = _forward_exact(C, x, cr, r, relu, clip,
                                                       f"{what} forward relu={relu} clip={clip} res={r is not None}", g)
    # eval apply from running statistics (mean, 1/4)
    rv = torch.full((c,), 0.25, device=DEV)
    for relu, clip, r in ((False, INF, None), (True, 6.0, res), (True, INF, None), (False, INF, res)):
        y, sm, si = C.bn_eval_apply(x, cr.mean, rv, cr.w, cr.b, 0.0, r, relu, c, clip)
        _, invstd, scale, shift = R.bn_eval_coeffs(cr.mean, rv, cr.w, cr.b, 0.0)
        w2 = f"{what} eval relu={relu} clip={clip} res={r is not None}"
        _exact(y, _stored(R.bn_apply(x, scale, shift, r, relu, clip), dtype, w2), w2)
        _exact(sm, cr.mean, w2 + " mean")
        _exact(si, invstd, w2 + " invstd")
    # finalize
    rm, rv0, nbt = cr.rm0.clone(), cr.rv0.clone(), torch.tensor([7], device=DEV)
    coef = C.bn_finalize(cr.sums, cr.w, cr.b, rm, rv0, 0.5, 0.0, c, nbt)
    _exact(coef, torch.stack([cr.scale, cr.shift, cr.coef[0], cr.coef[2]]), what + " finalize")
    _running_ok(rm, rv0, cr, what + " finalize")
    assert nbt.item() == 8
    # backward: no mask, mask from y (residual fused, both clips), mask from x (both clips)
    _backward_exact(C, dy, x, cr, 0, None, INF, g, what)
    for clip in (INF, 6.0):
        _backward_exact(C, dy, x, cr, 1, ys[(clip, True)], clip, g, f"{what} clip={clip}")
        _backward_exact(C, dy, x, cr, 2, None, clip, g, f"{what} clip={clip}")
    return g


@pytest.mark.parametrize("c,dtype,expect", S.CHANNEL_SPLIT, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_channel_split(c, dtype, expect):
    """One lane per row, idle lanes (tid / tc >= rpi), a full block of channel
    vectors, and a last channel chunk of a single lane: every kernel, with the
    weight, the bias or both absent as well (they are read from constants)."""
    C = _native.require("bn")
    torch.manual_seed(0)
    S.check_plan(C.bn_plan, S.CHANNEL_M, c, dtype, **expect)
    for weight, bias in ((True, True), (False, True), (True, False), (False, False)):
        _battery(C, S.CHANNEL_M, c, dtype, weight, bias)


@pytest.mark.parametrize("c,dtype,rpi,m_one_row", S.ROW_LOOPS)
def test_row_loops(c, dtype, rpi, m_one_row):
    """The 4-rows-in-flight loop of the moments kernel and its tail, the 2-row
    loop of the apply kernel and its single-row tail, slabs with fewer rows
    than the block has lane rows, a short last slab and a last slab of one row."""
    C = _native.require("bn")
    torch.manual_seed(1)
    assert C.bn_plan(1, c, dtype)["rpi"] == rpi
    ms = S.row_loop_ms(rpi)
    passes = set()
    for m in ms:
        g = _battery(C, m, c, dtype)
        passes.add(-(-g["rows_per_block"] // rpi))
    assert passes >= {1, 2, 3, 4, 5}, passes
    g = C.bn_plan(8 * rpi + 1, c, dtype)
    assert g["row_blocks"] == 2 and g["last_block_rows"] < g["rows_per_block"]
    if m_one_row is not None:
        g = _battery(C, m_one_row, c, dtype)
        assert g["row_blocks"] >= 2 and g["last_block_rows"] == 1


def _poisoned(n, k=8):
    """Frees k fp64 blocks of n elements full of NaN, each between two blocks
    that stay allocated (returned, to be kept until after the call), so that
    the caching allocator hands the next allocations of that size one of them.
    A free block of the same size that holds something else would be handed
    out first: two probe allocations find such blocks, which are then filled
    with NaN and kept too.  Returns (the poisoned pointers, keep)."""
    blocks = [torch.full((n,), float("nan"), dtype=F64, device=DEV) for _ in range(2 * k + 1)]
    ptrs = {t.data_ptr() for t in blocks[1::2]}
    keep = blocks[0::2]
    del blocks
    for _ in range(16):
        probes = [torch.empty(n, dtype=F64, device=DEV) for _ in range(2)]
        stray = [p for p in probes if p.data_ptr() not in ptrs]
        del probes
        if not stray:
            break
        for p in stray:
            p.fill_(float("nan"))
        keep += stray
        del stray, p
    return ptrs, keep


def _on_poison(call, n, pick, need, what):
    """Run `call` so that its [n] fp64 result lands on memory that holds NaN."""
    ptrs, keep = _poisoned(n)
    out = call()
    if need:
        assert pick(out).data_ptr() in ptrs, (
            f"{what}: the result was not allocated on the poisoned memory, so this run cannot tell whether "
            f"the kernel zeroes its sums before the atomic reduce adds to them")
    del keep
    return out


@pytest.mark.parametrize("m,c,dtype,rb,chunks,cchunks", S.PARTIAL_REDUCE)
def test_partial_reduce(m, c, dtype, rb, chunks, cchunks):
    """256 partial rows are stored; from 257 on the producer's block 0 zeroes the
    sums and each chunk of 256 rows adds with fp64 atomics.  The sums come from
    an uninitialised allocation, here one that holds NaN; on integers the order
    of the atomics cannot matter, so two runs agree bit for bit."""
    C = _native.require("bn")
    torch.manual_seed(2)
    g = S.check_plan(C.bn_plan, m, c, dtype, row_blocks=rb, reduce_chunks=chunks, cchunks=cchunks,
                     zeroed=int(rb > 256))
    need = bool(g["zeroed"])
    what = f"M={m} C={c} {dtype}"
    x, dy = _ints((m, c), dtype), _ints((m, c), dtype)
    cr = Crafted(c)
    first = lambda t: t
    _partials_fit(15, g, what)

    ref = R.bn_moments(x)
    for run in (1, 2):
        sums = _on_poison(lambda: C.bn_local_moments(x, c), 2 * c + 1, first, need, what + " moments")
        _exact(sums, ref, f"{what} moments run {run}")

    yr = _stored(R.bn_apply(x, cr.scale, cr.shift, None, True, 6.0), dtype, what)
    yk = yr.float().to(dtype)
    for mode in (0, 1, 2):
        mask = (None, R.bn_mask_from_y(yr, 6.0), R.bn_mask_from_x(x, cr.scale, cr.shift, 6.0))[mode]
        ref = R.bn_bwd_moments(dy, x, cr.mean, mask)
        for run in (1, 2):
            sums = _on_poison(lambda: C.bn_backward_moments(dy, x, yk if mode == 1 else None, cr.mean, mode != 0, c,
                                                            cr.w, cr.b, cr.invstd, 6.0),
                              2 * c, first, need, f"{what} backward moments mode {mode}")
            _exact(sums, ref, f"{what} backward moments mode {mode} run {run}")

    if dtype == BF16:
        _partials_fit(36, g, what)
        ref = R.bn_moments(yr)
        for run in (1, 2):
            out = _on_poison(lambda: C.bn_forward_apply(x, cr.sums, cr.w, cr.b, None, None, 0.5, 0.0, None, True, c,
                                                        None, True, 6.0),
                             2 * c + 1, lambda o: o[3], need, what + " output moments")
            _exact(out[0], yr, f"{what} y run {run}")
            _exact(out[3], ref, f"{what} output moments run {run}")


@pytest.mark.parametrize("m,c,dtype", [(37, 96, BF16), (2049, 2048, BF16), (300, 1028, F32)])
def test_mask_strictness(m, c, dtype):
    """Pre-activations exactly 0 and exactly 6 pass no gradient (0 < y < clip,
    both strict), whether the mask is read from the saved output or re-derived
    from x: forward, backward moments and backward apply equal the reference
    and each other."""
    C = _native.require("bn")
    torch.manual_seed(3)
    x, dy = _ints((m, c), dtype), _ints((m, c), dtype)
    cr = Crafted(c)
    # scale in {1, -1, 2} with shift 3, 3, 0: t = x*scale + shift takes 0 and 6 on every channel
    kind = torch.arange(c, device=DEV) % 3
    cr.w = torch.tensor([0.5, -0.5, 1.0], device=DEV)[kind]
    cr.coef = R.bn_fwd_coeffs(cr.sums, cr.w, None, 0.0)
    cr.b = (torch.tensor([3.0, 3.0, 0.0], device=DEV, dtype=F64)[kind] + cr.coef[0] * cr.coef[3]).float()
    cr.coef = R.bn_fwd_coeffs(cr.sums, cr.w, cr.b, 0.0)
    t = R.bn_preact(x, cr.scale, cr.shift)
    assert float((t == 0).double().mean()) >= 0.05 and float((t == 6).double().mean()) >= 0.05
    g = C.bn_plan(m, c, dtype)
    what = f"strict M={m} C={c} {dtype}"
    yr = _forward_exact(C, x, cr, None, True, 6.0, what, g)
    yk = yr.float().to(dtype)
    mask = R.bn_mask_from_y(yr, 6.0)
    assert torch.equal(mask, R.bn_mask_from_x(x, cr.scale, cr.shift, 6.0))
    assert torch.equal(mask, (t > 0) & (t < 6))
    ref = R.bn_bwd_moments(dy, x, cr.mean, mask)
    s1 = C.bn_backward_moments(dy, x, yk, cr.mean, True, c, cr.w, cr.b, cr.invstd, 6.0)
    s2 = C.bn_backward_moments(dy, x, None, cr.mean, True, c, cr.w, cr.b, cr.invstd, 6.0)
    _exact(s1, ref, what + " moments from y")
    _exact(s2, ref, what + " moments from x")
    assert torch.equal(s1, s2)
    a, b, cc, dwr, dbr = R.bn_bwd_coeffs(cr.bsums, COUNT, cr.w, cr.mean, cr.invstd, True)
    dxr, dzr = R.bn_bwd_apply(dy, x, a, b, cc, mask)
    _stored(dxr, dtype, what)
    o1 = C.bn_backward_apply(dy, x, yk, cr.bsums, cr.count, cr.w, cr.mean, cr.invstd, True, True, True, c, cr.b, 6.0)
    o2 = C.bn_backward_apply(dy, x, None, cr.bsums, cr.count, cr.w, cr.mean, cr.invstd, True, True, True, c, cr.b, 6.0)
    for o, src in ((o1, "y"), (o2, "x")):
        _exact(o[0], dxr, f"{what} dx from {src}")
        _exact(o[3], dzr, f"{what} dres from {src}")
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[3], o2[3])
    # a fused residual moves other elements onto the thresholds; the mask then comes from y alone
    res = _ints((m, c), dtype)
    _backward_exact(C, dy, x, cr, 1, _forward_exact(C, x, cr, res, True, 6.0, what + " residual", g), 6.0, g,
                    what + " residual")


@pytest.mark.parametrize("c,dtype", S.SHARD_CASES)
def test_split_phase_contract(c, dtype):
    """What SyncBatchNorm relies on: shards of unequal size, an empty one and a
    one-row one among them, compute local moments; their sum is the batch's;
    every shard applied with the summed moments and the global count gives the
    rows the whole batch gives."""
    C = _native.require("bn")
    torch.manual_seed(4)
    m = sum(S.SHARDS)
    x, dy, res = _ints((m, c), dtype), _ints((m, c), dtype), _ints((m, c), dtype)
    cr = Crafted(c)
    w = torch.randn(c, device=DEV)
    b = torch.randn(c, device=DEV)
    bounds, r0 = [], 0
    for n in S.SHARDS:
        bounds.append((r0, r0 + n))
        r0 += n
    full = C.bn_local_moments(x, c)
    _exact(full, R.bn_moments(x), "full moments")
    parts = [C.bn_local_moments(x[a:e], c) for a, e in bounds]
    assert torch.equal(torch.stack(parts).sum(0), full)
    assert full[2 * c].item() == m
    rm, rv = cr.rm0.clone(), cr.rv0.clone()
    y, sm, si = C.bn_forward_apply(x, full, w, b, rm, rv, 0.1, 1e-5, res, True, c, None, False, INF)
    fbm = C.bn_backward_moments(dy, x, y, cr.mean, True, c, None, None, None, INF)
    _exact(fbm, R.bn_bwd_moments(dy, x, cr.mean, R.bn_mask_from_y(y)), "full backward moments")
    count = torch.tensor([float(m)], dtype=F64, device=DEV)
    fdx, fdw, fdb, fdres = C.bn_backward_apply(dy, x, y, fbm, count, w, sm, si, True, True, True, c, b, INF)
    bparts = []
    for a, e in bounds:
        what = f"shard rows {a}:{e} C={c} {dtype}"
        rm_s, rv_s = cr.rm0.clone(), cr.rv0.clone()
        ys, sms, sis = C.bn_forward_apply(x[a:e], full, w, b, rm_s, rv_s, 0.1, 1e-5, res[a:e], True, c, None, False,
                                          INF)
        assert ys.shape == (e - a, c) and torch.equal(ys, y[a:e]), what
        if e > a:  # an empty shard launches nothing
            assert torch.equal(sms, sm) and torch.equal(sis, si), what
            assert torch.equal(rm_s, rm) and torch.equal(rv_s, rv), what
        bparts.append(C.bn_backward_moments(dy[a:e], x[a:e], ys, cr.mean, True, c, None, None, None, INF))
        if e == a:
            assert not parts[len(bparts) - 1].any() and not bparts[-1].any(), what
            assert parts[len(bparts) - 1].shape == (2 * c + 1,) and bparts[-1].shape == (2 * c,)
        dx, dw, db, dres = C.bn_backward_apply(dy[a:e], x[a:e], ys, fbm, count, w, sm, si, True, True, True, c, b,
                                               INF)
        assert dx.shape == (e - a, c) and dres.shape == (e - a, c)
        assert torch.equal(dx, fdx[a:e]) and torch.equal(dres, fdres[a:e]), what
        if e > a:
            assert torch.equal(dw, fdw) and torch.equal(db, fdb), what
    assert torch.equal(torch.stack(bparts).sum(0), fbm)


def _sliced_exact(out, ref_of, what, rows=16384):
    """out [M, C] against ref_of(row0, row1) in slices, so that no fp64 copy of the whole tensor exists."""
    for r in range(0, out.shape[0], rows):
        _exact(out[r:r + rows], ref_of(r, min(out.shape[0], r + rows)), f"{what} rows {r}+")


@pytest.mark.parametrize("case", ["bf16_res_relu_dres", "bf16_out_moments", "f32_no_dres"])
def test_non_temporal(case):
    """M*C*2 >= 256 MiB takes the non-temporal loads and stores of the forward
    apply, the forward apply with output moments and the backward apply: exact,
    and bit for bit what the cached instantiations give."""
    C = _native.require("bn")
    torch.manual_seed(5)
    m, c = S.STREAMING
    dtype = F32 if case.startswith("f32") else BF16
    assert C.bn_plan(m, c, dtype)["streaming"] == 1
    assert C.bn_plan(*S.NOT_STREAMING, dtype)["streaming"] == 0
    g = C.bn_plan(m, c, dtype)
    cr = Crafted(c)
    x = _ints((m, c), dtype)
    with_res = case == "bf16_res_relu_dres"
    res = _ints((m, c), dtype) if with_res else None
    clip = INF if with_res else 6.0
    dy = _ints((m, c), dtype) if case != "bf16_out_moments" else None
    mode = 1 if with_res else 2

    def run():
        fwd = C.bn_forward_apply(x, cr.sums, cr.w, cr.b, None, None, 0.5, 0.0, res, True, c, None,
                                 case == "bf16_out_moments", clip)
        if dy is None:
            return [fwd[0], fwd[3]]
        bwd = C.bn_backward_apply(dy, x, fwd[0] if mode == 1 else None, cr.bsums, cr.count, cr.w, cr.mean, cr.invstd,
                                  True, True, with_res, c, cr.b, clip)
        return [fwd[0], bwd[0], bwd[1], bwd[2]] + ([bwd[3]] if with_res else [])

    outs = run()
    sl = lambda t, a, e: None if t is None else t[a:e]
    yref = lambda a, e: _stored(R.bn_apply(x[a:e], cr.scale, cr.shift, sl(res, a, e), True, clip), dtype, case)
    _sliced_exact(outs[0], yref, case + " y")
    if dy is None:
        _partials_fit(36, g, case)
        ref = torch.zeros(2 * c + 1, dtype=F64, device=DEV)
        for r in range(0, m, 16384):
            ref += R.bn_moments(yref(r, r + 16384))
        _exact(outs[1], ref, case + " output moments")
    else:
        a_, b_, c_, dwr, dbr = R.bn_bwd_coeffs(cr.bsums, COUNT, cr.w, cr.mean, cr.invstd, True)

        def bref(a, e):
            mask = R.bn_mask_from_y(yref(a, e), clip) if mode == 1 else \
                R.bn_mask_from_x(x[a:e], cr.scale, cr.shift, clip)
            return R.bn_bwd_apply(dy[a:e], x[a:e], a_, b_, c_, mask)
        _sliced_exact(outs[1], lambda a, e: _stored(bref(a, e)[0], dtype, case), case + " dx")
        _exact(outs[2], dwr, case + " dweight")
        _exact(outs[3], dbr, case + " dbias")
        if with_res:
            _sliced_exact(outs[4], lambda a, e: bref(a, e)[1], case + " dres")
    C.set_bn_streaming(False)
    try:
        assert C.bn_plan(m, c, dtype)["streaming"] == 0
        cached = run()
    finally:
        C.set_bn_streaming(True)
    assert C.bn_plan(m, c, dtype)["streaming"] == 1
    for i, (o, k) in enumerate(zip(outs, cached)):
        assert torch.equal(o, k), f"{case}: output {i} differs between the non-temporal and the cached kernels"


def _real_case(m, c, dtype, dead=False):
    """randn data with per-channel offsets of 0, 4 and 16 standard deviations;
    with `dead`, channel 1 is all zero and channel 2 constant (77/256, which is
    0.3 as bf16 holds it: the sums of at most 37 such values are exact in fp32,
    so its batch mean is the value itself and its variance is 0)."""
    x = torch.randn(m, c, device=DEV) + torch.tensor([0.0, 4.0, 16.0], device=DEV)[torch.arange(c, device=DEV) % 3]
    if dead:
        x[:, 1] = 0.0
        x[:, 2] = 77.0 / 256.0
        assert 5929 * m < 2 ** 24
    return (x.to(dtype), torch.randn(m, c, device=DEV).to(dtype), torch.randn(m, c, device=DEV).to(dtype),
            torch.randn(c, device=DEV), torch.randn(c, device=DEV))


def _real_checks(C, m, c, dtype, dead):
    g = C.bn_plan(m, c, dtype)
    n = g["rows_per_block"]
    what = f"real M={m} C={c} {dtype}" + (" dead channels" if dead else "")
    x, dy, res, w, b = _real_case(m, c, dtype, dead)
    eps = 1e-5
    dead_ch = [1, 2] if dead else []
    # moments against fp64
    sums = C.bn_local_moments(x, c)
    ref = R.bn_moments(x)
    sa, qa = R.bn_moments_abs(x)
    _within(sums[:c], ref[:c], n * R.U * sa, what + " sum")
    _within(sums[c:2 * c], ref[c:2 * c], (n + 1) * R.U * qa, what + " sum of squares")
    assert sums[2 * c].item() == m
    # apply against the reference fed the kernel's own moments
    mean, var, invstd, scale, shift = R.bn_fwd_coeffs(sums, w, b, eps)
    saved = None
    for relu, clip, r in ((False, INF, None), (True, 6.0, None), (True, INF, res)):
        w2 = f"{what} forward relu={relu} clip={clip} res={r is not None}"
        y, sm, si = C.bn_forward_apply(x, sums, w, b, None, None, 0.1, eps, r, relu, c, None, False, clip)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(sm).all()) and bool(torch.isfinite(si).all())
        yr = R.bn_apply(x, scale, shift, r, relu, clip)
        bound = 8 * R.U * R.bn_apply_abs(x, mean, scale, b, r) + _half_ulp(yr, dtype)
        _within(y, yr, bound, w2)
        # one rounding to fp32 of a value the kernel forms in fp64 (U), and that fp64 arithmetic's own noise
        _within(sm, mean, 2 * R.U * mean.abs(), w2 + " save_mean")
        _within(si, invstd, 2 * R.U * invstd, w2 + " save_invstd")
        for ch in dead_ch:  # a dead channel normalises to its bias
            at_bias = b[ch].double() + (r[:, ch].double() if r is not None else 0.0)
            at_bias = at_bias.clamp(0.0, clip) if relu else at_bias
            _within(y[:, ch], at_bias.expand(m), bound[:, ch], f"{w2} channel {ch} at its bias")
        saved = (y, sm, si)
    if dead:  # the kernel's own moments give a variance of exactly 0: invstd = 1/sqrt(eps)
        assert var[1].item() == 0.0 and var[2].item() == 0.0
    # backward, with the mean and invstd the forward saved; the mask from the stored y is unambiguous
    y, sm, si = saved
    a_scale = (w.double() * si.double())
    a_shift = b.double() - sm.double() * a_scale
    t = R.bn_preact(x, a_scale, a_shift)
    tb = 8 * R.U * R.bn_apply_abs(x, sm.double(), a_scale, b)
    count = torch.tensor([float(m)], dtype=F64, device=DEV)
    for mode, clip in ((0, INF), (1, INF), (2, 6.0)):
        w2 = f"{what} backward mode {mode}"
        if mode == 2:  # elements within the pre-activation's own bound of a threshold may go either way
            unsure = (t.abs() <= tb) | ((t - clip).abs() <= tb)
            assert float(unsure.double().mean()) < 1e-4, w2
            mask = R.bn_mask_from_x(x, a_scale, a_shift, clip)
        else:
            unsure = torch.zeros_like(t, dtype=torch.bool)
            mask = None if mode == 0 else R.bn_mask_from_y(y, clip)
        yk = y if mode == 1 else None
        bs = C.bn_backward_moments(dy, x, yk, sm, mode != 0, c, w, b, si, clip)
        br = R.bn_bwd_moments(dy, x, sm, mask)
        ba, bq = R.bn_bwd_moments_abs(dy, x, sm, mask)
        ua, uq = R.bn_bwd_moments_abs(dy, x, sm, unsure)  # what a flipped element moves the sums by
        _within(bs[:c], br[:c], n * R.U * ba + ua, w2 + " sum dz")
        qbound = (n + 2) * R.U * bq + uq  # x - mean is rounded before the multiply-add
        _within(bs[c:], br[c:], qbound, w2 + " sum dz*(x-mean)")
        a, bb, cc, dwr, dbr = R.bn_bwd_coeffs(bs, m, w, sm, si, True)
        dx, dw, db, dres = C.bn_backward_apply(dy, x, yk, bs, count, w, sm, si, True, mode != 0, True, c, b, clip)
        assert all(bool(torch.isfinite(o).all()) for o in (dx, dw, db, dres)), w2
        dxr, dzr = R.bn_bwd_apply(dy, x, a, bb, cc, mask)
        bound = 8 * R.U * R.bn_bwd_apply_abs(dy, x, a, bb, cc, mask) + _half_ulp(dxr, dtype)
        keep = ~unsure
        _within(dx[keep], dxr[keep], bound[keep], w2 + " dx")
        _exact(dres[keep], dzr[keep], w2 + " dres")
        _within(dw, dwr, 2 * R.U * dwr.abs(), w2 + " dweight")
        _within(db, dbr, 2 * R.U * dbr.abs(), w2 + " dbias")
        for ch in dead_ch:  # x - mean is 0 on a dead channel: no weight gradient
            _within(dw[ch:ch + 1], torch.zeros(1, dtype=F64, device=DEV),
                    (qbound[ch:ch + 1] * si[ch].double()) * (1 + R.U), f"{w2} dweight of channel {ch}")


@pytest.mark.parametrize("m,c,dtype", S.REAL_SHAPES)
def test_real_data_within_fp32_fma_bounds(m, c, dtype):
    """Integers cannot show low-precision accumulation or a cancelling
    variance; randn data with channel means of up to 16 standard deviations,
    under bounds derived from fp32 arithmetic, does."""
    C = _native.require("bn")
    torch.manual_seed(6)
    _real_checks(C, m, c, dtype, dead=False)


@pytest.mark.parametrize("m,c,dtype", S.DEAD_SHAPES)
def test_dead_channels(m, c, dtype):
    """An all-zero and a constant channel among randn ones, eps = 1e-5: the
    variance clamps at 0, invstd = 1/sqrt(eps), everything stays finite, y sits
    at the bias, the weight gradient at 0 and dx within its bound."""
    C = _native.require("bn")
    torch.manual_seed(7)
    _real_checks(C, m, c, dtype, dead=True)
