"""GPU: the LayerNorm kernels (csrc/layernorm.hip) at every dispatch boundary, against float64, judged per row and per column.

Which kernel serves a call is decided by shape, dtype and arguments alone (launch_ln_fwd / launch_ln_bwd; the VITK_LN* switches are
compiled out of the product build), so every branch that ships is reached in process:

 A. forward: ln_fwd_kernel in each MAXC bucket (edges D = 256 / 768 / 1024 / 1280 / 2048 / 4096), ln_fwd_any_kernel (D % 4 != 0),
    ln_fwd16_kernel (16-bit x, y, w; D = 768 / 1024 / 1280; rows >= 1024), row maps, the position add, rows = 0;
 B. the forward's fp8 side output (y8 under a device scale, the amax64 record), whose grid is capped at 1,024 blocks;
 C. backward: ln_bwd_fast_kernel (f32 stream, 16-bit stream, dropout), ln_bwd_kernel (no gin / no dx column sums / row maps / the
    MAXC bucket widths), ln_bwd_any_kernel (narrow and wide), the partial rows and both folds;
 D. edge-value rows mixed into the tensors of A and C: constant rows, |mean| / std of 10 / 100 / 1000, spread ~ sqrt(eps),
    magnitude 1e4, zero-dy rows, eps 1e-5 and 1e-6;
 E. the patch-embedding LayerNorm (patch_ln_fwd / patch_ln_bwd_params) across its 32,768-patch grid cap.

Row counts are chosen so that every wave walks several rows (the forward grid is at most occupancy x CUs blocks of 4 waves, the
backward grid is capped by vitk_layernorm_bwd_blocks), and so that a walk ends one row short of / on / one row past a full pass.

Every cell: outputs pre-filled with NaN sentinel bit patterns inside guard rows (and the rows a row map skips), every element the
call must write finite afterwards, every guard / skipped element unchanged, each row (y, mean, rstd, dx_f32, dx_t) and each
column (dw, db, dcol) held to the existing whole-tensor gate of test_kernels_gpu.py on its own, the whole tensor too, and two
runs bit-identical."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from vit_pytorch_amd import _lib as L  # noqa: E402
from vit_pytorch_amd import kernels as K  # noqa: E402
from vit_pytorch_amd import ops  # noqa: E402

DEV = "cuda"
BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U = 2.0 ** -24                      # unit roundoff of float32
EPS = ops.LN_EPS

# ---- gates: the existing whole-tensor gates of test_kernels_gpu.py ------------------------------------------------------
G_Y = {F32: 2e-6, BF: 4e-3, F16: 4e-3}          # y (test_layernorm_fwd)
G_DXF = 3e-6                                    # dx_f32 (test_layernorm_bwd)
G_DXT = {F32: 3e-6, BF: 4e-3, F16: 4e-3}        # dx_t
G_STAT = 1e-5                                   # mean, rstd
G_W = {F32: 1e-5, BF: 5e-3, F16: 5e-3}          # dw, db in the parameter dtype (whole vector)
G_W32 = 1e-5                                    # dw, db folded in float32 (test_layernorm_bwd with float32 parameters,
                                                # test_patch_ln_gather_fwd_and_param_grads): the partial rows are float32 sums of
                                                # the same summands whatever the parameter dtype
G_DCOL = 1e-4                                   # dcol (column sums of dx_t)

SENT = {1: 0x7F, 2: 0x7FA5, 4: 0x7FBADBAD}      # NaN bit patterns (e4m3fn, bf16 / f16, f32) that no kernel writes
IDT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
GUARD = 8                                       # sentinel rows before and after every output (keeps a view of D % 4 == 0
                                                # columns 16-byte aligned, as the vector kernels require)

REPORT = {}                                     # (section, dtype, quantity) -> (worst err / gate, err, gate, cell)
F8_MISMATCH = {}                                # dtype -> y8 elements that differ from round-to-nearest-even of the float64 value


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def randn(shape, g, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


def bits(t):
    return t.view(IDT[t.element_size()])


def dname(d):
    return {F32: "f32", BF: "bf16", F16: "f16"}[d]


def record(sec, dt, q, err, gate, tag):
    k = (sec, dname(dt), q)
    r = err / gate if gate > 0 else (0.0 if err == 0 else math.inf)
    if k not in REPORT or r > REPORT[k][0]:
        REPORT[k] = (r, err, gate, tag)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k in sorted(REPORT):
        r, e, g, tag = REPORT[k]
        print(f"[ln-summary] {k[0]} {k[1]} {k[2]}: worst {e:.2e} / gate {g:.2e} ({r:.2f} of the gate) at {tag}")
    for k, n in sorted(F8_MISMATCH.items()):
        print(f"[ln-summary] B {k} y8: {n} elements off round-to-nearest-even of the float64 value, all near a midpoint")


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Out:
    """An output of n rows x D inside a store with GUARD sentinel rows on either side.  `live`: the rows of the view the call
    must write (all by default; a row map's skipped rows are not live).  fill() writes the sentinel everywhere (NaN-prefill),
    check() asserts the live rows finite and everything else unchanged."""

    def __init__(self, n, D, dtype, live=None):
        self.store = torch.empty(n + 2 * GUARD, D, dtype=dtype, device=DEV)
        self.v = self.store[GUARD:GUARD + n]
        self.vec = self.v[:, 0] if D == 1 else None
        self.live = torch.zeros(n + 2 * GUARD, dtype=torch.bool, device=DEV)
        if live is None:
            self.live[GUARD:GUARD + n] = True
        else:
            self.live[GUARD + live] = True
        self.sent = SENT[self.store.element_size()]
        self.zero = False                                       # amax64: the live words start at 0 (atomicMax records)

    def t(self):
        return self.vec if self.vec is not None else self.v

    def fill(self):
        bits(self.store).fill_(self.sent)
        if self.zero:
            self.v.zero_()

    def check(self, tag, name):
        b = bits(self.store)
        assert (b[~self.live] == self.sent).all(), (tag, name, "a guard / skipped row was written")
        if self.store.dtype == torch.uint8:                   # e4m3fn: 0x7F / 0xFF are its only NaNs
            ok = ((b[self.live] & 0x7F) != 0x7F).all()
        else:
            ok = torch.isfinite(self.store[self.live].float()).all()
        assert ok, (tag, name, "non-finite (unwritten) entries")


def twice(tag, outs, call):
    """Run `call` twice, each time on freshly NaN-filled outputs; the two runs must agree bit for bit.  Returns after the second."""
    first = None
    for _ in range(2):
        for o in outs.values():
            o.fill()
        call()
        snap = {n: bits(o.store).clone() for n, o in outs.items()}
        if first is None:
            first = snap
    for n in outs:
        assert torch.equal(first[n], snap[n]), (tag, n, "differs between two identical runs")
    for n, o in outs.items():
        o.check(tag, n)


def map_rows(m, rows):
    """Store rows of logical rows 0..rows-1 under RowMap m (common.h map_row)."""
    r = torch.arange(rows, device=DEV)
    if m.group <= 0:
        return r
    return (r // m.group) * m.gstride + r % m.group + m.offset


# ---- inputs with edge-value rows (D) -------------------------------------------------------------------------------------
def const_value(D):
    """A constant whose float32 row mean the kernels form exactly: every partial sum k * c is exact (c has two significant bits,
    D <= 4096), and (D * c) * fl(1 / D) must round back to c -- the kernels multiply by invD = 1.0f / D."""
    inv = torch.tensor(1.0, dtype=F32) / D
    for c in (0.75, -1.5, 1.0, -0.5, 3.0, 0.375, -2.0):
        if (torch.tensor(c * D, dtype=F32) * inv).item() == c:
            return c
    raise AssertionError(f"no exact constant for D = {D}")


EDGE_MIN_ROWS = 64


def make_x(rows, D, dtype, seed, eps=EPS, edges=True):
    """x (rows, D) of `dtype`: randn * 2 + 0.5 rows (the existing tests' inputs) with one row of each edge kind mixed in when there
    are at least EDGE_MIN_ROWS rows (the last row is a constant one as well).  Returns x, {kind: row index}, ratio (float64 per row:
    |mean| / std where that exceeds 1, 0 elsewhere -- the factor the derived gates of the offset rows carry; a row of 3 or 5
    random elements can land there too, and the same derivation holds for it)."""
    g = gen(seed)
    x = randn((rows, D), g, 2.0) + 0.5
    kinds = {}
    ratio = torch.zeros(rows, dtype=F64, device=DEV)
    if edges and rows >= EDGE_MIN_ROWS:
        ks = ["const", "tiny", "big"] + (["off10", "off100", "off1000"] if dtype == F32 else [])
        for i, k in enumerate(ks):
            kinds[k] = int((i + 0.5) * rows / len(ks))
        kinds["const_last"] = rows - 1
        for k, r in kinds.items():
            if k.startswith("const"):
                x[r] = const_value(D)
            elif k == "tiny":
                x[r] = randn((D,), g, math.sqrt(eps))                   # spread ~ sqrt(eps): var + eps ~ 2 eps
            elif k == "big":
                x[r] = randn((D,), g, 1e4).clamp(-3e4, 3e4)             # representable in bf16 and in f16 (max 65504)
            else:
                m = float(k[3:])
                x[r] = randn((D,), g) + (m if r % 2 else -m)
    x = x.to(dtype)
    if rows:
        xd = x.double()
        m, sd = xd.mean(-1).abs(), xd.std(-1, unbiased=False)
        ratio = torch.where((sd > 0) & (m > sd), m / sd.clamp_min(1e-300), ratio)
    return x, kinds, ratio


def params(D, wdt, seed, bias=True):
    g = gen(seed)
    w = (1 + 0.1 * randn((D,), g)).to(wdt)
    b = (0.1 * randn((D,), g)).to(wdt) if bias else None
    return w, b


def ln64(xd, w, b, eps):
    """float64 LayerNorm of float64 rows; eps as the kernel sees it (a float32)."""
    e = float(torch.tensor(eps, dtype=F32))
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + e)
    xh = (xd - mu) * rs
    y = xh * w.double() + (b.double() if b is not None else 0.0)
    return y, mu[:, 0], rs[:, 0], xh


def row_err(got, ref, den=None):
    e = (got.double() - ref).norm(dim=1)
    n = ref.norm(dim=1) if den is None else den
    return e, e / n.clamp_min(1e-300)


def judge_rows(sec, dt, q, tag, got, ref, base, ratio, derived_slope, den=None, plain=None, floor=None):
    """Each row: ||got_r - ref_r|| / ||ref_r|| (or / den_r) <= base + derived_slope * ratio_r (+ floor_r / ||ref_r||).  ratio_r is
    non-zero only on rows whose |mean| exceeds their spread (make_x); floor_r (dx): see bwd_cell.  Both derived where they are passed.  `plain` selects the rows
    held to the unchanged whole-tensor gate `base` as a whole."""
    e, r = row_err(got, ref, den)
    n = ref.norm(dim=1) if den is None else den
    gate = base + derived_slope * ratio
    if floor is not None:
        gate = gate + floor / n.clamp_min(1e-300)
    q_ = r / gate
    i = int(q_.argmax())
    record(sec, dt, q, r[i].item(), gate[i].item(), f"{tag} row {i}")
    assert (r <= gate).all(), (tag, q, "row", i, r[i].item(), gate[i].item())
    if plain is None:
        plain = ratio == 0
    if plain.any():
        whole = e[plain].norm().item() / max(ref[plain].norm().item(), 1e-300)
        assert whole < base, (tag, q, "whole tensor", whole, base)


def judge_stats(sec, tag, mean, rstd, mu, rs, kinds, ratio, eps, dt):
    """mean: |mean_r - mu_r| <= G_STAT * rms(x_r) -- the float32 sum's rounding grows with the row's magnitude, not with |mean_r|
    (a row of mean ~0 has no relative scale of its own); rstd: relative, G_STAT.  Constant rows: mean exact (const_value),
    rstd within one float32 ulp of 1 / sqrt(eps)."""
    em = (mean.double() - mu).abs()
    rms = torch.sqrt(mu * mu + 1.0 / (rs * rs) - float(torch.tensor(eps, dtype=F32)))
    rm = em / rms.clamp_min(1e-300)
    i = int(rm.argmax())
    record(sec, dt, "mean", rm[i].item(), G_STAT, f"{tag} row {i}")
    assert (rm <= G_STAT).all(), (tag, "mean", i, rm[i].item())
    er = ((rstd.double() - rs) / rs).abs()
    i = int(er.argmax())
    record(sec, dt, "rstd", er[i].item(), G_STAT, f"{tag} row {i}")
    assert (er <= G_STAT).all(), (tag, "rstd", i, er[i].item())
    # the whole-tensor gate of the existing tests (relative to ||mean||) over the ordinary rows; below EDGE_MIN_ROWS rows it is a
    # per-row figure of a handful of rows whose mean may lie near 0, where the per-row gate above is the meaningful one
    plain = ratio == 0
    if int(plain.sum()) >= EDGE_MIN_ROWS:
        assert (mean.double() - mu)[plain].norm().item() < G_STAT * mu[plain].norm().item(), (tag, "mean whole")
    # constant rows: var = 0, rstd = 1.0f / sqrtf(0 + eps) -- a correctly rounded square root and a correctly rounded division, each
    # off by at most u relative: 2u of 1 / sqrt(eps) (at eps = 1e-6 that is 1.02 ulp of the float32 result, 1000 sits low in its binade)
    r_true = 1.0 / math.sqrt(float(torch.tensor(eps, dtype=F32)))
    for k, r in kinds.items():
        if k.startswith("const"):
            d = abs(rstd[r].double().item() - r_true) / r_true
            record(sec, dt, "rstd (constant rows)", d, 2 * U, f"{tag} row {r}")
            assert d <= 2 * U, (tag, k, "rstd of a constant row", rstd[r].item(), r_true)


# ---- A / B / D: forward ---------------------------------------------------------------------------------------------------
def fwd_cell(sec, tag, rows, D, xdt, ydt, wdt, seed, eps=EPS, bias=True, imap=None, omap=None, add_mode=None, Np=None,
             f8=None, scale=96.0):
    """One forward call through K.layernorm_fwd, judged.  imap / omap: RowMap or None; add_mode: None, 'pos' (add_group = Np,
    add_off = 1: the position embedding at patch rows) or 'rows' (one add row per row); f8: None, 'y8', 'amax', 'y8_amax'."""
    x, kinds, ratio = make_x(rows, D, xdt, seed, eps)
    w, b = params(D, wdt, seed + 1, bias)
    im, om = imap or L.IDENT, omap or L.IDENT
    xin = x
    if imap is not None:                                        # the skipped input rows hold NaN: reading one poisons a row
        src_rows = map_rows(im, rows)
        xin = torch.full((int(src_rows.max()) + 2, D), float("nan"), dtype=xdt, device=DEV)
        xin[src_rows] = x
    elif rows == 0:                                            # rows = 0 on real allocations (an empty tensor's pointer is null)
        xin = torch.zeros(1, D, dtype=xdt, device=DEV)
    dst_rows = map_rows(om, rows)
    ny = int(dst_rows.max()) + 1 if rows else 1                 # rows = 0: one output row, not live
    add = None
    ag, ao = 0, 0
    g = gen(seed + 2)
    if add_mode == "pos":
        add = randn((Np + 1, D), g, 0.5).to(wdt)
        ag, ao = Np, 1
        addr = add.double()[torch.arange(rows, device=DEV) % Np + 1]
    elif add_mode == "rows":
        add = randn((rows, D), g, 0.5).to(wdt)
        addr = add.double()
    nst = max(rows, 1)
    outs = {"y": Out(ny, D, ydt, live=dst_rows), "mean": Out(nst, 1, F32, live=torch.arange(rows, device=DEV)),
            "rstd": Out(nst, 1, F32, live=torch.arange(rows, device=DEV))}
    sc = None
    if f8 in ("y8", "y8_amax"):
        outs["y8"] = Out(ny, D, torch.uint8, live=dst_rows)
        sc = torch.tensor([scale], dtype=F32, device=DEV)
    if f8 in ("amax", "y8_amax"):
        outs["amax64"] = Out(64, 1, F32)
        outs["amax64"].zero = True

    def call():
        K.layernorm_fwd(xin, w, b, outs["y"].t(), outs["mean"].t(), outs["rstd"].t(), rows, D, eps, im, om, add, ag, ao,
                        outs["y8"].t() if "y8" in outs else None, sc, outs["amax64"].t() if "amax64" in outs else None)

    twice(tag, outs, call)
    if rows == 0:
        return
    y = outs["y"].v[dst_rows]
    ref, mu, rs, xh = ln64(x.double(), w, b, eps)
    if add is not None:
        ref = ref + addr
    # per-row gate: the whole-tensor gate, + the float32 gate x |mean| / std on rows whose |mean| exceeds their spread (the offset
    # rows of D): the float32 sum that forms the mean is off by ~u |mean|, which shifts every x_hat of the row by u |mean| / std --
    # no float32 computation of the mean does better
    judge_rows(sec, ydt, "y", tag, y, ref, G_Y[ydt], ratio, G_Y[F32])
    judge_stats(sec, tag, outs["mean"].t(), outs["rstd"].t(), mu, rs, kinds, ratio, eps, xdt)
    for k, r in kinds.items():
        if k.startswith("const"):                       # x_hat = 0 exactly: y = b (+ add) exactly, rounded once
            assert outs["mean"].t()[r].item() == const_value(D), (tag, k, "mean not exact")
            exp = (b.float() if b is not None else torch.zeros(D, device=DEV))
            if add is not None:
                exp = exp + addr[r].float()
            assert torch.equal(y[r], exp.to(ydt)), (tag, k, "y != b")
    if f8 is not None:
        judge_f8(sec, tag, ydt, outs, dst_rows, ref, xh, mu.abs() * rs, w, b, addr if add is not None else None, sc)
    return dict(outs=outs, y=y, ref=ref, x=x, w=w, b=b)


def judge_f8(sec, tag, ydt, outs, dst_rows, ref, xh, mr, w, b, addr, sc):
    if "y8" in outs:
        s = sc.item()
        dec = outs["y8"].v[dst_rows].view(torch.float8_e4m3fn).float().double()
        t = (ref * s).clamp(-448.0, 448.0)                                 # the clamp is exact
        e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -6)))         # e4m3: 3 mantissa bits, subnormal step 2^-9
        step = torch.exp2(e - 3)
        # float32 error of the kernel's y * scale: (x - mean) * rstd * w + b (+ add) with the statistics a few ulps off -- 64 ulps of
        # the terms' magnitudes, x_hat's counted as |x_hat| + |mean| / std (the float32 mean is off by ~u |mean|, which moves x_hat
        # by u |mean| / std: on the offset rows of D that is more than an e4m3 step of a small value)
        tol = 64 * U * s * ((xh.abs() + mr[:, None]) * w.double().abs() + (b.double().abs() if b is not None else 0.0)
                            + (addr.abs() if addr is not None else 0.0))
        off = (dec - t).abs() > step + tol                                  # tol << step except on the offset rows
        assert not off.any(), (tag, "y8 more than one e4m3 step off", off.nonzero()[:4].tolist(), dec[off][:4].tolist(), t[off][:4].tolist())
        q = t / step
        rne = torch.round(q) * step                                         # round-half-even of the float64 value
        mism = dec != rne
        # the kernel rounds its float32 value: it may disagree with round-to-nearest-even of the float64 value only where that value
        # lies within the float32 error of a rounding midpoint
        dist = ((q - torch.floor(q)) - 0.5).abs() * step
        bad = mism & (dist > tol)
        n_m = int(mism.sum())
        print(f"[ln-f8] {tag}: {n_m} of {dec.numel()} y8 elements differ from RNE of the float64 value")
        F8_MISMATCH[dname(ydt)] = F8_MISMATCH.get(dname(ydt), 0) + n_m
        assert not bad.any(), (tag, "y8 differs from RNE away from a midpoint", int(bad.sum()), bad.nonzero()[:4].tolist())
    if "amax64" in outs:
        words = outs["amax64"].t().double()
        assert torch.isfinite(words).all() and (words >= 0).all(), (tag, "amax64 words")
        m = words.max().item()
        r = ref.abs().max().item()
        record(sec, ydt, "amax", abs(m - r) / r, 1e-5, tag)
        assert abs(m - r) <= 1e-5 * r, (tag, "amax", m, r)


FWD_DT = [(F32, F32, F32), (F32, BF, BF), (F32, F32, BF), (BF, BF, BF), (BF, F32, BF), (F16, F16, F16)]
BUCKET_D = [4, 252, 256, 260, 764, 768, 772, 1020, 1024, 1028, 1276, 1280, 1284, 2044, 2048, 2052, 4092, 4096]
ANY_D = [3, 5, 147, 1323, 3199]
ROWS_SMALL = [1, 3, 4, 5, 1023]
# several passes of every wave at ANY occupancy: the forward grid is at most 8,192 blocks (launch_ln_fwd) of 4 waves = 32,768 rows,
# and at most (32 waves per CU) x CUs waves -- test_big_row_counts_walk checks the latter on the device at hand
ROWS_BIG = [50432, 50433, 65537]


def fwd_cells():
    for xdt, ydt, wdt in FWD_DT:
        for D in BUCKET_D + ANY_D:
            for rows in ROWS_SMALL + [50433]:
                yield xdt, ydt, wdt, D, rows
            if (xdt, ydt, wdt) in ((F32, BF, BF), (F16, F16, F16)):
                for rows in (50432, 65537):
                    yield xdt, ydt, wdt, D, rows


def test_big_row_counts_walk():
    cus = cu_count()
    for rows in ROWS_BIG:
        assert rows >= 32 * cus + 1 and rows > 8192 * 4, (rows, cus)


@pytest.mark.parametrize("xdt,ydt,wdt,D,rows", list(fwd_cells()),
                         ids=lambda v: dname(v) if isinstance(v, torch.dtype) else str(v))
def test_fwd_matrix(xdt, ydt, wdt, D, rows):
    fwd_cell("A", f"fwd {dname(xdt)}/{dname(ydt)}/{dname(wdt)} D={D} rows={rows}", rows, D, xdt, ydt, wdt, seed=1000 + D + rows)


@pytest.mark.parametrize("dt", [BF, F16], ids=dname)
@pytest.mark.parametrize("D", [768, 1024, 1280])
@pytest.mark.parametrize("rows", [1023, 1024, 1025, 1026, 1031, 50432, 50433, 50439])
@pytest.mark.parametrize("bias", [True, False])
def test_fwd16_rows(dt, D, rows, bias):
    """ln_fwd16_kernel from 1,024 rows (1,023: still the general kernel); per row it must match the general kernel fed the same
    values in float32 to 2 output ulps of the row's largest value (2 x 2^-8 relative for bf16, 2 x 2^-10 for f16)."""
    tag = f"fwd16 {dname(dt)} D={D} rows={rows} bias={bias}"
    c = fwd_cell("A", tag, rows, D, dt, dt, dt, seed=2000 + D + rows, bias=bias)
    x, w, b, y, ref = c["x"], c["w"], c["b"], c["y"], c["ref"]
    y2 = torch.empty(rows, D, dtype=dt, device=DEV)
    m2 = torch.empty(rows, device=DEV); r2 = torch.empty(rows, device=DEV)
    K.layernorm_fwd(x.float(), w, b, y2, m2, r2, rows, D)                 # float32 x: ln_fwd_kernel
    ulp = 2.0 ** -8 if dt == BF else 2.0 ** -10
    d = (y.double() - y2.double()).abs().amax(1)
    lim = 2 * ulp * ref.abs().amax(1)
    i = int((d / lim).argmax())
    assert (d <= lim).all(), (tag, "row", i, d[i].item(), lim[i].item())


@pytest.mark.parametrize("dt", [(F32, F32, F32), (F32, BF, BF), (BF, BF, BF), (F16, F16, F16)],
                         ids=lambda t: "-".join(dname(d) for d in t))
@pytest.mark.parametrize("D", [768, 64, 147])
@pytest.mark.parametrize("B,Np", [(256, 196), (3, 6)])
@pytest.mark.parametrize("mode", ["omap_pos", "omap", "imap_cls", "imap_omap", "add_rows"])
def test_fwd_rowmaps_and_add(dt, D, B, Np, mode):
    """Row maps with a cls slot (omap: patch rows -> rows 1..Np of each (B, N, D) image, row 0 skipped), imap reading the cls rows,
    the position add (add_group = Np, add_off = 1) and a plain per-row add."""
    xdt, ydt, wdt = dt
    N = Np + 1
    tag = f"fwd maps {mode} {'/'.join(dname(d) for d in dt)} D={D} B={B}"
    cls_map, patch_map = L.RowMap(1, N, 0), L.RowMap(Np, N, 1)
    if mode == "omap_pos":
        fwd_cell("A", tag, B * Np, D, xdt, ydt, wdt, seed=3000 + D, omap=patch_map, add_mode="pos", Np=Np)
    elif mode == "omap":
        fwd_cell("A", tag, B * Np, D, xdt, ydt, wdt, seed=3001 + D, omap=patch_map)
    elif mode == "imap_cls":
        fwd_cell("A", tag, B, D, xdt, ydt, wdt, seed=3002 + D, imap=cls_map)
    elif mode == "imap_omap":
        fwd_cell("A", tag, B * Np, D, xdt, ydt, wdt, seed=3003 + D, imap=patch_map, omap=patch_map)
    else:
        fwd_cell("A", tag, B * Np, D, xdt, ydt, wdt, seed=3004 + D, add_mode="rows")


@pytest.mark.parametrize("dt", [F32, BF, F16], ids=dname)
@pytest.mark.parametrize("D", [768, 147])
def test_fwd_empty_batch(dt, D):
    """rows = 0 (functional._empty_batch_forward's batch): success, nothing written."""
    fwd_cell("A", f"fwd empty {dname(dt)} D={D}", 0, D, dt, dt, dt, seed=5)


def test_fwd_refusals():
    x = torch.zeros(4, 4100, device=DEV)
    w = torch.ones(4100, device=DEV)
    y = torch.empty_like(x); m = torch.empty(4, device=DEV); r = torch.empty(4, device=DEV)
    with pytest.raises(L.VitkError):
        K.layernorm_fwd(x[:, :4097].contiguous(), w[:4097], None, y[:, :4097].contiguous(), m, r, 4, 4097)
    x = torch.zeros(8, 147, dtype=BF, device=DEV); w = torch.ones(147, dtype=BF, device=DEV); y = torch.empty_like(x)
    y8 = torch.empty(8, 147, dtype=torch.uint8, device=DEV); sc = torch.ones(1, device=DEV)
    am = torch.zeros(64, dtype=torch.int32, device=DEV)
    m = torch.empty(8, device=DEV); r = torch.empty(8, device=DEV)
    with pytest.raises(L.VitkError):
        K.layernorm_fwd(x, w, None, y, m, r, 8, 147, y8=y8, scale8=sc)
    with pytest.raises(L.VitkError):
        K.layernorm_fwd(x, w, None, y, m, r, 8, 147, amax64=am)


@pytest.mark.parametrize("dt", [(BF, BF, BF), (F32, BF, BF), (F16, F16, F16)], ids=lambda t: "-".join(dname(d) for d in t))
@pytest.mark.parametrize("D", [768, 1280, 1024])
@pytest.mark.parametrize("rows", [4095, 4096, 4097, 50433])
@pytest.mark.parametrize("maps", [False, True])
@pytest.mark.parametrize("f8", ["y8_amax", "y8", "amax"])
def test_fwd_fp8_side_output(dt, D, rows, maps, f8):
    """B: y8 (e4m3 of y * scale, clamped at +-448) and the amax64 record.  With amax64 the grid is capped at 1,024 blocks of 4 waves:
    4,096 rows is the walk boundary.  maps: the patch-embedding form (omap with a cls slot + the position add)."""
    xdt, ydt, wdt = dt
    tag = f"fp8 {f8} {'/'.join(dname(d) for d in dt)} D={D} rows={rows} maps={maps}"
    if maps:
        Np = 196 if rows % 196 == 0 else rows                           # rows = B * Np; a prime row count: one image of Np rows
        fwd_cell("B", tag, rows, D, xdt, ydt, wdt, seed=4000 + D + rows, omap=L.RowMap(Np, Np + 1, 1), add_mode="pos", Np=Np, f8=f8)
    else:
        fwd_cell("B", tag, rows, D, xdt, ydt, wdt, seed=4000 + D + rows, f8=f8)


@pytest.mark.parametrize("kern", ["general_f32", "general_bf16", "any", "fwd16_bf16", "fwd16_f16"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_fwd_edge_rows_eps(kern, eps):
    """D: the edge rows under eps 1e-5 (ops.LN_EPS) and 1e-6 in each forward kernel, at a row count where every wave walks."""
    xdt, ydt, wdt, D = {"general_f32": (F32, F32, F32, 1024), "general_bf16": (F32, BF, BF, 768), "any": (F32, F32, F32, 1323),
                        "fwd16_bf16": (BF, BF, BF, 768), "fwd16_f16": (F16, F16, F16, 1280)}[kern]
    fwd_cell("D", f"fwd edge {kern} eps={eps}", 50433, D, xdt, ydt, wdt, seed=6000, eps=eps)


# ---- C / D: backward ------------------------------------------------------------------------------------------------------
def walk_edge(D):
    """One full pass of the backward grid, read from vitk_layernorm_bwd_blocks: the block count it stops growing at times the
    waves per block (the row count at which it first returns 2, minus one) -- 4,096 narrow, 3,072 wide."""
    nw = next(r for r in range(1, 65) if K.layernorm_bwd_blocks(r + 1, D) == 2)
    return K.layernorm_bwd_blocks(1 << 40, D) * nw


def resolve(rows, D):
    """Row counts are given as ints or as 'E-1' / 'E' / 'E+1' around walk_edge(D) (resolved on the device, not at collection)."""
    if isinstance(rows, int):
        return rows
    return walk_edge(D) + int(rows[1:] or 0)


def bwd_cell(sec, tag, rows, D, dyt, xdt, wdt, stream="f32", p=0.0, variant="plain", seed=0, eps=EPS):
    """One backward call, judged.  stream: 'f32' (K.layernorm_bwd: dx_f32 + dx_t) or 's16' (K.layernorm_bwd_s16: dx_t is the
    16-bit stream).  variant: 'plain' (gin, both dx outputs, dx column sums, identity maps: the fast kernel's case at D = 768 / 1024 /
    1280), 'nogin', 'nocol', 'dxt_only' (no dx_f32), 'maps' (dy, x, dx and gin through RowMap(G, G + 1, 1))."""
    x, kinds, ratio = make_x(rows, D, xdt, seed, eps)
    w, _ = params(D, wdt, seed + 1, bias=False)
    g = gen(seed + 2)
    dy = randn((rows, D), g)
    zero_rows = []
    if rows >= EDGE_MIN_ROWS:
        zero_rows = [rows // 3, kinds.get("const", 0)]               # a zero-dy row on its own and on a constant row
        dy[zero_rows] = 0.0
    dy = dy.to(dyt)
    s16 = stream == "s16"
    gdt = dyt if s16 else F32
    gin = None if variant == "nogin" else randn((rows, D), g).to(gdt)
    tdt = F32 if wdt == F32 else wdt
    colsum = variant != "nocol"
    m = L.RowMap(7, 8, 1) if variant == "maps" else L.IDENT
    srows = map_rows(m, rows)
    nst = int(srows.max()) + 2

    def stored(t):                                    # logical rows placed at their mapped rows, NaN in the skipped ones
        if variant != "maps" or t is None:
            return t
        s = torch.full((nst, D), float("nan"), dtype=t.dtype, device=DEV)
        s[srows] = t
        return s

    dy_s, x_s, gin_s = stored(dy), stored(x), stored(gin)
    ndx = nst if variant == "maps" else rows
    xd = x.double()
    _, mu, rs, xh = ln64(xd, w, None, eps)
    mean, rstd = mu.float(), rs.float()
    nblk = K.layernorm_bwd_blocks(rows, D)
    outs = {"dx_t": Out(ndx, D, tdt, live=srows), "partials": Out(3 * nblk, D, F32, live=torch.arange((3 if colsum else 2) * nblk, device=DEV))}
    if not s16 and variant != "dxt_only":
        outs["dx_f32"] = Out(ndx, D, F32, live=srows)
    fold = {"dw32": F32, "db32": F32, "dwt": tdt, "dbt": tdt, "cw32": F32, "cb32": F32, "cwt": tdt, "cbt": tdt}
    if colsum:
        fold.update({"dc32": F32, "dct": tdt, "cc32": F32, "cct": tdt})
    for n, d in fold.items():
        outs[n] = Out(D, 1, d)

    def call():
        P = outs["partials"].store[GUARD:GUARD + 3 * nblk].flatten()
        if s16:
            K.layernorm_bwd_s16(dy_s, x_s, w, mean, rstd, gin_s, outs["dx_t"].v, P, colsum, rows, D, m, m, m)
        else:
            K.layernorm_bwd(dy_s, x_s, w, mean, rstd, gin_s, outs["dx_f32"].v if "dx_f32" in outs else None, outs["dx_t"].v, P,
                            colsum, rows, D, m, m, m, drop_p=p, drop_seed=seed)
        K.layernorm_bwd_finalize(P, nblk, D, outs["dw32"].t(), outs["db32"].t(), outs["dc32"].t() if colsum else None, L.F32)
        K.layernorm_bwd_finalize(P, nblk, D, outs["dwt"].t(), outs["dbt"].t(), outs["dct"].t() if colsum else None, K.dt(tdt))
        for s, nm in enumerate(["w", "b"] + (["c"] if colsum else [])):
            K.colsum_partials(P[s * nblk * D:], nblk, D, D, outs[f"c{nm}32"].t())
            K.colsum_partials(P[s * nblk * D:], nblk, D, D, outs[f"c{nm}t"].t())

    twice(tag, outs, call)

    # float64 reference from the same stored inputs (the closed form of LayerNorm's autograd backward, test_bwd_closed_form)
    dyd = dy.double()
    gw = dyd * w.double()
    c1 = gw.mean(-1, keepdim=True)
    c2 = (gw * xh).mean(-1, keepdim=True)
    dxl = rs[:, None] * (gw - c1 - xh * c2)
    dx = dxl + (gin.double() if gin is not None else 0.0)
    keepf = None
    if p > 0:
        kb = torch.empty(ndx, D, dtype=torch.uint8, device=DEV)
        K.dropout_keep(kb, ndx, D, p, seed)
        keepf = kb[srows].double() / (1 - p)
    dxm = dx * keepf if keepf is not None else dx
    # per-row gates: the whole-tensor gates; offset rows: + the float32 gate x |mean| / std -- the float32 mean handed to the kernel
    # is itself rounded by up to u |mean|, which moves every x_hat of the row by u |mean| / std, and x_hat enters dx linearly, so no
    # float32 computation does better.  Constant rows (x_hat = 0, dx = rstd (g - mean(g))) are measured against rstd ||dy w||.
    den = dx.norm(dim=1).clone()
    special = ratio != 0
    for k, r in kinds.items():
        if k.startswith("const"):
            den[r] = max(den[r].item(), rs[r].item() * gw[r].norm().item())
            special[r] = True
    plain = ~special
    # dx_r = rstd (g - c1 - x_hat c2) + gin: its float32 evaluation errs relative to the magnitudes of these terms, a few roundings
    # each -- 8u of their norm, added to the gate.  Negligible (< 1/6 of the float32 gate) unless the terms cancel, which happens
    # on rows of 3 or 5 elements (dx of a LayerNorm row sums to 0 and is orthogonal to x_hat: 1 and 3 degrees of freedom)
    mr = (mu.abs() * rs)[:, None]
    mdx = rs[:, None] * (gw.abs() + c1.abs() + (xh.abs() + mr) * c2.abs()) + (gin.double().abs() if gin is not None else 0.0)
    if "dx_f32" in outs:
        judge_rows(sec, F32, "dx_f32", tag, outs["dx_f32"].v[srows], dx, G_DXF, ratio, G_DXF, den=den, plain=plain,
                   floor=8 * U * mdx.norm(dim=1))
    dent = den
    if keepf is not None:
        dent = dxm.norm(dim=1).clone()
        for k, r in kinds.items():
            if k.startswith("const"):
                dent[r] = max(dent[r].item(), rs[r].item() * (gw[r] * keepf[r]).norm().item())
    judge_rows(sec, tdt, "dx_t", tag, outs["dx_t"].v[srows], dxm, G_DXT[tdt], ratio, G_DXF, den=dent, plain=plain,
               floor=8 * U * (mdx * keepf if keepf is not None else mdx).norm(dim=1))
    # zero-dy rows: dx is exactly the incoming gradient (dropout-masked and scaled in float32 for dx_t)
    if gin is not None:
        inv = (torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))).item()
        for r in zero_rows:
            gr = gin[r].float()
            if "dx_f32" in outs:
                assert torch.equal(outs["dx_f32"].v[srows[r]], gr), (tag, "zero-dy row", r, "dx_f32 != gin")
            exp = gr if keepf is None else torch.where(keepf[r] > 0, gr * inv, torch.zeros_like(gr))
            assert torch.equal(outs["dx_t"].v[srows[r]], exp.to(tdt)), (tag, "zero-dy row", r, "dx_t != gin")
    # columns: each column of the float32 folds against g * ||m_c||_2, m_rc the magnitude of its float64 summand t_rc as float32
    # forms it -- a summand's float32 error is relative to the quantities it is made of, not to the summand, which may cancel:
    #   dw: dy (|x_hat| + |mean| / std)   (the float32 mean is off by ~u |mean|: x_hat by u |mean| / std -- the offset rows of D)
    #   db: |dy|                          (exact summands)
    #   dcol: keep (rstd (|dy w| + |c1| + (|x_hat| + |mean| / std) |c2|) + |gin|)   (dx's own terms)
    # With many rows this is ||t_c||_2 up to a factor ~1 + |mean| / std (1.25 on the ordinary rows, randn * 2 + 0.5).
    terms = {"w": (dyd * xh, dyd.abs() * (xh.abs() + mr)), "b": (dyd, dyd.abs())}
    if colsum:
        terms["c"] = (dxm, mdx * keepf if keepf is not None else mdx)
    for nm, (t, mag) in terms.items():
        ref = t.sum(0)
        scale = mag.norm(dim=0)
        gc = G_DCOL if nm == "c" else G_W32
        for src in (f"d{nm}32", f"c{nm}32"):
            e = (outs[src].t().double() - ref).abs()
            r = e / scale.clamp_min(1e-300)
            i = int(r.argmax())
            record(sec, dyt, f"d{nm} (col, f32 fold)", r[i].item(), gc, f"{tag} col {i}")
            assert (e <= gc * scale).all(), (tag, src, "column", i, r[i].item(), gc)
        # both folds agree bit for bit; the parameter-dtype outputs are the float32 fold rounded once
        assert torch.equal(bits(outs[f"d{nm}32"].store), bits(outs[f"c{nm}32"].store)), (tag, nm, "finalize vs colsum_partials")
        assert torch.equal(bits(outs[f"d{nm}t"].store), bits(outs[f"c{nm}t"].store)), (tag, nm, "finalize vs colsum_partials, T")
        assert torch.equal(outs[f"d{nm}t"].t(), outs[f"d{nm}32"].t().to(tdt)), (tag, nm, "T fold != rounded f32 fold")
        # the existing whole-vector gates
        gw_ = G_DCOL if nm == "c" else G_W[tdt]
        src = outs["dc32"].t() if nm == "c" else outs[f"d{nm}t"].t()
        wv = (src.double() - ref).norm().item() / max(ref.norm().item(), 1e-300)
        assert wv < gw_, (tag, nm, "whole vector", wv, gw_)


BWD_DT = [(F32, F32, F32), (BF, F32, BF), (BF, BF, BF), (F32, F32, BF), (F32, BF, BF), (F16, F16, F16), (F16, F32, F16)]


def bwd_rows(few=False):
    if few:
        return [9, "E", "E+1", 50433]
    return [1, 7, 8, 9, "E-1", "E", "E+1", 50432, 50433]


def ids_dt(t):
    return "-".join(dname(d) for d in t)


def fast_cells():
    for D in (768, 1024, 1280):
        for dt in BWD_DT:
            for rows in bwd_rows():
                yield D, dt, "f32", 0.0, rows
                if dt[0] != F32 and dt[2] != F32:
                    yield D, dt, "s16", 0.0, rows
            for p in (0.1, 0.5):
                for rows in bwd_rows(few=True):
                    yield D, dt, "f32", p, rows


@pytest.mark.parametrize("D,dt,stream,p,rows", list(fast_cells()), ids=lambda v: ids_dt(v) if isinstance(v, tuple) else str(v))
def test_bwd_fast(D, dt, stream, p, rows):
    """ln_bwd_fast_kernel: gin, both dx outputs (or the 16-bit stream), dx column sums, identity maps, D = 768 / 1024 / 1280;
    dropout: dx_f32 unmasked, dx_t and dcol masked by K.dropout_keep's decisions."""
    dyt, xdt, wdt = dt
    rows = resolve(rows, D)
    bwd_cell("C", f"bwd fast {ids_dt(dt)} D={D} {stream} p={p} rows={rows}", rows, D, dyt, xdt, wdt, stream, p, seed=7000 + D + rows)


def general_cells():
    dts = [(F32, F32, F32), (BF, F32, BF), (BF, BF, BF), (F16, F16, F16)]
    for D in (768, 1024, 1280):
        for dt in dts:
            for variant in ("nogin", "nocol", "dxt_only", "maps"):
                for rows in (9, "E+1", 50433):
                    yield D, dt, "f32", variant, rows
                    if dt[0] != F32 and variant != "dxt_only":
                        yield D, dt, "s16", variant, rows
    for D in BUCKET_D:
        if D in (768, 1024, 1280):
            continue
        for dt in dts:
            for rows in (9, "E+1", 50433):
                yield D, dt, "f32", "plain", rows
                if dt[0] != F32:
                    yield D, dt, "s16", "plain", rows


@pytest.mark.parametrize("D,dt,stream,variant,rows", list(general_cells()), ids=lambda v: ids_dt(v) if isinstance(v, tuple) else str(v))
def test_bwd_general(D, dt, stream, variant, rows):
    """ln_bwd_kernel: the fast kernel's widths reached by leaving out gin, the dx column sums or dx_f32, or through row maps; and
    every MAXC bucket width (one row each side of the bucket edges) with the full set of outputs."""
    dyt, xdt, wdt = dt
    rows = resolve(rows, D)
    bwd_cell("C", f"bwd general {ids_dt(dt)} D={D} {stream} {variant} rows={rows}", rows, D, dyt, xdt, wdt, stream, 0.0, variant,
             seed=8000 + D + rows)


def any_cells():
    for D in (3, 5, 147, 1323, 3197, 3199):
        for dt in [(F32, F32, F32), (BF, F32, BF), (BF, BF, BF), (F16, F16, F16)]:
            for rows in (1, 9, "E-1", "E", "E+1", 50433):
                yield D, dt, 0.0, "plain", rows
            yield D, dt, 0.3, "plain", "E+1"
            yield D, dt, 0.0, "maps", "E+1"
            yield D, dt, 0.0, "nocol", 50433


@pytest.mark.parametrize("D,dt,p,variant,rows", list(any_cells()), ids=lambda v: ids_dt(v) if isinstance(v, tuple) else str(v))
def test_bwd_any(D, dt, p, variant, rows):
    """ln_bwd_any_kernel (D % 4 != 0): the narrow form (8 waves, D < 768) and the wide one (4 waves), LDS accumulators."""
    dyt, xdt, wdt = dt
    rows = resolve(rows, D)
    bwd_cell("C", f"bwd any {ids_dt(dt)} D={D} p={p} {variant} rows={rows}", rows, D, dyt, xdt, wdt, "f32", p, variant,
             seed=9000 + D + rows)


@pytest.mark.parametrize("kern", ["fast_f32", "fast_s16", "general", "any"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_bwd_edge_rows_eps(kern, eps):
    """D: the edge rows under eps 1e-5 and 1e-6 in each backward kernel, every wave walking."""
    D, dt, stream, variant = {"fast_f32": (768, (F32, F32, F32), "f32", "plain"), "fast_s16": (1280, (BF, BF, BF), "s16", "plain"),
                              "general": (1024, (F32, F32, BF), "f32", "nogin"), "any": (1323, (F32, F32, F32), "f32", "plain")}[kern]
    bwd_cell("D", f"bwd edge {kern} eps={eps}", 50433, D, *dt, stream, 0.0, variant, seed=9500, eps=eps)


def test_bwd_refusals():
    D = 3201                                            # D % 4 != 0 beyond 3,200: the LDS accumulators would not fit
    x = torch.zeros(8, D, device=DEV); dy = torch.zeros(8, D, device=DEV); w = torch.ones(D, device=DEV)
    m = torch.zeros(8, device=DEV); r = torch.ones(8, device=DEV)
    part = torch.empty(3 * K.layernorm_bwd_blocks(8, D) * D, device=DEV)
    with pytest.raises(L.VitkError):
        K.layernorm_bwd(dy, x, w, m, r, None, torch.empty_like(x), None, part, True, 8, D)
    D = 147                                             # the 16-bit stream needs D % 4 == 0
    x = torch.zeros(8, D, dtype=BF, device=DEV); w = torch.ones(D, dtype=BF, device=DEV)
    with pytest.raises(L.VitkError):
        K.layernorm_bwd_s16(x, x, w, m, r, None, torch.empty_like(x), part, True, 8, D)


def test_bwd_closed_form():
    """The closed form bwd_cell's reference uses is LayerNorm's float64 autograd backward."""
    D, rows = 147, 40
    x, _, _ = make_x(rows, D, F32, 1)
    w, b = params(D, F32, 2)
    dy = randn((rows, D), gen(3))
    xd = x.double().requires_grad_(True); wd = w.double().requires_grad_(True); bd = b.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (D,), wd, bd, EPS).backward(dy.double())
    _, mu, rs, xh = ln64(x.double(), w, b, EPS)
    gw = dy.double() * w.double()
    dx = rs[:, None] * (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True))
    assert torch.allclose(dx, xd.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose((dy.double() * xh).sum(0), wd.grad, rtol=1e-12, atol=1e-12)


# ---- E: the patch-embedding LayerNorm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, F16], ids=dname)
@pytest.mark.parametrize("B,H,W", [(1, 224, 224), (2, 224, 224), (167, 224, 224), (168, 224, 224), (256, 224, 224), (3, 48, 80),
                                   (5, 16, 16)])
@pytest.mark.parametrize("bias", [True, False])
def test_patch_ln(dt, B, H, W, bias):
    """patch_ln_fwd (grid capped at 4,096 blocks x 8 patches = 32,768 patches per pass: B = 168 at 224^2 is the first batch that
    walks) and patch_ln_bwd_params against float64 patchify + LayerNorm; a constant, a tiny-spread and a 1e4 patch in the last
    image.  Each patch row and each gamma / beta column judged on its own."""
    C, p, P = 3, 16, 768
    tag = f"patch {dname(dt)} B={B} {H}x{W} bias={bias}"
    g = gen(11000 + B + H + W)
    img = randn((B, C, H, W), g, 1.5) + 0.2
    img[-1, :, :16, :16] = const_value(P)                           # patch 0 of the last image
    if W >= 32:
        img[-1, :, :16, 16:32] = randn((C, 16, 16), g, math.sqrt(EPS))
    if H >= 32:
        img[-1, :, 16:32, :16] = randn((C, 16, 16), g, 1e4).clamp(-3e4, 3e4)
    img = img.to(dt)
    w, b = params(P, dt, 11001, bias)
    h, ww = H // p, W // p
    rows = B * h * ww
    assert K.patch_ln_serves(img, C, H, W, p, p)
    outs = {"y": Out(rows, P, dt), "mean": Out(rows, 1, F32), "rstd": Out(rows, 1, F32)}
    twice(tag, outs, lambda: K.patch_ln_fwd(img, w, b, outs["y"].v, outs["mean"].t(), outs["rstd"].t(), B, C, H, W, p, p))
    patches = img.double().reshape(B, C, h, p, ww, p).permute(0, 2, 4, 3, 5, 1).reshape(rows, P)
    ref, mu, rs, xh = ln64(patches, w, b, EPS)
    zero = torch.zeros(rows, dtype=F64, device=DEV)
    judge_rows("E", dt, "y", tag, outs["y"].v, ref, G_Y[dt], zero, 0.0)
    r0 = (B - 1) * h * ww
    judge_stats("E", tag, outs["mean"].t(), outs["rstd"].t(), mu, rs, {"const": r0}, zero, EPS, dt)
    assert outs["mean"].t()[r0].item() == const_value(P), (tag, "constant patch mean")
    assert torch.equal(outs["y"].v[r0], b if b is not None else torch.zeros(P, dtype=dt, device=DEV)), (tag, "constant patch y != b")
    # backward: dgamma / dbeta partial rows, folded in float32
    dy = randn((rows, P), g).to(dt)
    nblk = K.patch_ln_bwd_blocks(rows)
    mean, rstd = outs["mean"].t().clone(), outs["rstd"].t().clone()
    bo = {"partials": Out(2 * nblk, P, F32), "dw": Out(P, 1, F32), "db": Out(P, 1, F32)}

    def call():
        Pt = bo["partials"].store[GUARD:GUARD + 2 * nblk].flatten()
        K.patch_ln_bwd_params(dy, img, mean, rstd, Pt, B, C, H, W, p, p)
        K.colsum_partials(Pt, nblk, P, P, bo["dw"].t())
        K.colsum_partials(Pt[nblk * P:], nblk, P, P, bo["db"].t())

    twice(tag + " bwd", bo, call)
    for nm, t in (("dw", dy.double() * xh), ("db", dy.double())):
        refc = t.sum(0)
        scale = t.norm(dim=0)
        e = (bo[nm].t().double() - refc).abs()
        r = e / scale
        i = int(r.argmax())
        record("E", dt, f"{nm} (col)", r[i].item(), G_W32, f"{tag} col {i}")
        assert (e <= G_W32 * scale).all(), (tag, nm, "column", i, r[i].item())
        assert (e.norm() / refc.norm()).item() < G_W32, (tag, nm, "whole vector")


def test_patch_ln_refusals():
    img = torch.zeros(2, 3, 32, 32, dtype=BF, device=DEV)
    assert not K.patch_ln_serves(img.float(), 3, 32, 32, 16, 16)           # float32 images
    assert not K.patch_ln_serves(img, 1, 32, 32, 16, 16)                   # one channel
    assert not K.patch_ln_serves(img, 3, 32, 32, 14, 14)                   # 14 x 14 patches
    assert not K.patch_ln_serves(img, 3, 40, 32, 16, 16)                   # H % 16 != 0
    assert not K.patch_ln_serves(img, 3, 32, 40, 16, 16)                   # W % 16 != 0
    assert not K.patch_ln_serves(img, 3, 32, 32, 16, 8)                    # non-square patches
    y = torch.empty(8, 768, dtype=BF, device=DEV); m = torch.empty(8, device=DEV); r = torch.empty(8, device=DEV)
    w = torch.ones(768, dtype=BF, device=DEV)
    with pytest.raises(L.VitkError):
        K.patch_ln_fwd(img, w, None, y, m, r, 2, 3, 32, 32, 14, 14)
    with pytest.raises(L.VitkError):
        K.patch_ln_bwd_params(y, img, m, r, torch.empty(2 * 768, device=DEV), 2, 1, 32, 32, 16, 16)
