"""GPU: the 16-bit GEMMs at every dispatch boundary, against float64 products of the same stored operands, judged per element.

Entry points: vitk_gemm_nt_bf16 / _drop / _gelu_bwd_colsum / _mul_aux_colsum / _mul_aux8_colsum (C = A . W^T + epilogue) and
vitk_gemm_tn_bf16 / _pair (dW = dY^T X).  Which kernel serves an NT call is decided by gemm_nt_impl / nt_persist_dispatch
(csrc/gemm_bf16.hip) from the shape, ldc, the alignment of aux, the epilogue, the CU reserve and VITK_NT_W128:

  small  -- gemm_nt_kernel (128-row tiles): M < 1024, N < 256, N % 8 == 4, ldc % 8 == 4, or an aux that is 8- but not 16-byte aligned;
  256pp  -- gemm_nt256pp_kernel (fm = 7 or 8 m-fragments): the shapes above N = 16,128 that ntp_plan refuses;
  8-wave -- gemm_ntp_kernel alone: every other shape the persistent plan takes (K < 256, K % 64 != 0, N % 256 != 0, no column sums
            promised under dropout, VITK_NT_W128=0);
  split  -- gemm_ntw (four-wave kernel) on gemm_ntw_split()'s 256-row tiles, then the 8-wave kernel on the rest (>= 1,024 rows) with
            drop_m0 = rows_w and its partial rows behind the four-wave launch's.

Sections: A routing, B every epilogue on every route that serves it (refusals must raise VitkError), C column-sum partials, D CU
reserve 0 / 32 / 192, VITK_NT_W128=0 and the K-blocked W (bit identity), E fused dropout across the row split, F edge values mixed
into A and W (zero, 1e3 and cancelling rows), G the TN weight gradients, H the IEEE-half library on a subset of A, B, E and G.

Every cell: C, aux and partials / ws prefilled with NaN (the uint8 gelu' codes with 255, a byte no kernel writes) inside guard rows
(and guard columns where ldc > N), every written element finite afterwards, every guard unchanged, two runs bit-identical.

Gates.  The f32 accumulation of K exact products (16-bit x 16-bit fits in 24 bits) in any order is off by at most
gamma_K * S, gamma_K = K u32 / (1 - K u32), S = sum_k |a_k| |w_k| (the float64 product |A| @ |W|^T).  One more rounding to unit
roundoff u of a value whose exact neighbour v is within e leaves it within e + u (|v| + e) (rnd() below).  Each epilogue chains its
own roundings on top (derived at its gate); the GELU polynomial (csrc/gemm_nt_epi.h, q_phi_parts8) is off the exact Phi by at most
E_PHI = 2.05e-5 and its derivative form by E_DG_IN = 2.05e-5 inside the clamp |x| <= 4.5 and E_DG_OUT = 8.7e-5 outside it (measured
in float64 on a 1.2e-5 grid of [-12, 12]; we take 2.1e-5 / 8.8e-5).  A 32-wide K-step lost or read twice moves an element by about
sqrt(32) |a||w|, two orders of magnitude above these gates at every K tested.  Each (row, 256-column tile) is also held to the
existing whole-tensor gates (4e-3 for 16-bit outputs, 1e-5 for f32), and so is the whole tensor."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from vit_pytorch_amd import _lib as L  # noqa: E402
from vit_pytorch_amd import kernels as K  # noqa: E402

DEV = "cuda"
BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U32 = 2.0 ** -24
U16 = {BF: 2.0 ** -8, F16: 2.0 ** -11}
TINY = {BF: 2.0 ** -133, F16: 2.0 ** -25, F32: 2.0 ** -149}     # half the smallest subnormal: the absolute floor of one rounding
E_PHI, E_DG_IN, E_DG_OUT = 2.1e-5, 2.1e-5, 8.8e-5
G_T16, G_T32 = 4e-3, 1e-5                                      # the existing whole-tensor gates (test_kernels_gpu.py)
# Outputs rounded to the 16-bit type twice (GELU of the rounded pre-activation; GELU_BWD / MUL_AUX(8) of the rounded accumulator):
# per (row, 256-column tile) twice the whole-tensor gate.  A tile's relative error is weighted by its few largest elements, and one
# rounding alone reaches u16 = 3.9e-3 relative per element (measured on an MI355X: 4.07e-3 to 4.22e-3 for MUL_AUX tiles of 256
# columns, 7.6e-3 for GELU tiles of 8 columns whose pre-activations lie below 0, where x gelu'(x) / gelu(x) amplifies the first
# rounding).  The whole tensor stays at 4e-3, and every element at its derived gate.
G_T16_2 = 2 * 4e-3
G_COL = 1e-5                                                   # column sums of C (test_kernels_gpu.py::test_gemm_gelu_bwd_colsum)

SENT = {1: 0xFF, 2: 0x7FA5, 4: 0x7FBADBAD}                     # guard / prefill bit patterns: 255 (uint8 codes), NaN (16 / 32-bit)
IDT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
GUARD = 8
RESERVES = (0, 32, 192)

REPORT = {}                                                    # (section, dtype, quantity) -> (worst err / gate, cell)
MIDPOINTS = {}                                                 # dtype -> DG8 codes one off rne(200 gelu'(pre)) + 27, all near a midpoint


def dname(d):
    return {F32: "f32", BF: "bf16", F16: "f16"}[d]


def record(sec, dt, q, ratio, tag):
    k = (sec, dname(dt), q)
    if k not in REPORT or ratio > REPORT[k][0]:
        REPORT[k] = (ratio, tag)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k in sorted(REPORT):
        r, tag = REPORT[k]
        print(f"[gemm-summary] {k[0]} {k[1]} {k[2]}: worst per-element error {r:.3f} of its gate at {tag}")
    for k, n in sorted(MIDPOINTS.items()):
        print(f"[gemm-summary] B {k} DG8: {n[0]} of {n[1]} codes one off rne(200 gelu'(pre)) + 27, all within the polynomial's error of a midpoint")


@pytest.fixture(autouse=True)
def _reset_switches():
    yield
    os.environ.pop("VITK_NT_W128", None)
    os.environ.pop("VITK_TN_PAIR", None)
    set_reserve(0)


def set_reserve(c):
    K.set_cu_reserve(c)                 # each library flavour keeps its own reserve
    K.set_cu_reserve(c, F16)


def grid():
    """Resident workgroups of the persistent NT kernels (the device's CU count rounded down to a multiple of 8)."""
    g = K.gemm_nt_plan(4096, 256, 256, 256)["workgroups"]
    assert g > 0 and g % 8 == 0 and g <= torch.cuda.get_device_properties(0).multi_processor_count
    return g


def bits(t):
    return t.view(IDT[t.element_size()])


def gamma(n):
    return n * U32 / (1 - n * U32)


def rnd(v, e, u):
    """A value within e of exact v, rounded once to unit roundoff u, is within this of v."""
    return e + u * (v + e)


# ---- buffers with guards ------------------------------------------------------------------------------------------------------
class Out:
    """rows x cols (leading dimension ld >= cols) inside a store with GUARD sentinel rows above and below."""

    def __init__(self, rows, cols, ld, dtype, off=0):
        self.store = torch.empty((rows + 2 * GUARD) * ld + off, dtype=dtype, device=DEV)
        self.v = self.store[off + GUARD * ld:off + (GUARD + rows) * ld].view(rows, ld)[:, :cols]
        self.live = torch.zeros_like(self.store, dtype=torch.bool)
        self.live[off + GUARD * ld:off + (GUARD + rows) * ld].view(rows, ld)[:, :cols] = True
        self.sent = SENT[self.store.element_size()]

    def fill(self):
        bits(self.store).fill_(self.sent)

    def check(self, tag):
        b = bits(self.store)
        assert (b[~self.live] == self.sent).all(), (tag, "a guard element was written")
        if self.store.dtype == torch.uint8:
            assert (b[self.live] != 0xFF).all(), (tag, "unwritten gelu' codes")
        else:
            assert torch.isfinite(self.store[self.live].float()).all(), (tag, "non-finite (unwritten) entries")


def twice(tag, outs, call):
    """Run `call` twice on freshly prefilled outputs; both runs must agree bit for bit.  Returns the bits of the second."""
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
        o.check(f"{tag} {n}")
    return snap


# ---- operands with edge rows (F) -----------------------------------------------------------------------------------------------
_OPS = {}


def edge_rows(M):
    """Row indices of the edge kinds in a matrix of M rows (M >= 64)."""
    return {"zero": M // 7, "big": 2 * M // 7, "cancel": 3 * M // 7, "near": 4 * M // 7, "zero_last": M - 1}


def operand(rows, Kd, dtype, seed, role):
    """A (role 'a': rows of tokens) or W (role 'w': rows of output features) of N(0, 1) / N(0, 1/K) values with edge rows:
    zero rows, a row of magnitude 1e3 (A), and cancelling rows -- A rows [u, u] (exactly) and [u, u + d] (nearly) against W rows
    [w, -w]: their products sum to 0 / to a small remainder of terms up to 1e2 x larger.  Cached by (rows, K, dtype, seed, role)."""
    key = (rows, Kd, dtype, seed, role)
    if key in _OPS:
        return _OPS[key]
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn(rows, Kd, generator=g, device=DEV)
    if role == "w":
        x *= Kd ** -0.5
    kinds = {}
    if rows >= 64:
        kinds = edge_rows(rows)
        h = Kd // 2
        x[kinds["zero"]] = 0
        x[kinds["zero_last"]] = 0
        if role == "a":
            x[kinds["big"]] *= 1e3
            u = torch.randn(h, generator=g, device=DEV) * 30
            x[kinds["cancel"], :h] = u
            x[kinds["cancel"], h:] = u
            x[kinds["near"], :h] = u
            x[kinds["near"], h:] = u + torch.randn(h, generator=g, device=DEV) * 0.05
        else:
            w = torch.randn(h, generator=g, device=DEV) * Kd ** -0.5
            x[kinds["cancel"], :h] = w
            x[kinds["cancel"], h:] = -w
            x[kinds["near"], :h] = w
            x[kinds["near"], h:] = -w
    x = x.to(dtype)
    _OPS[key] = (x, kinds)
    return _OPS[key]


_REFS = {}


def products(A, W, key):
    """float64 A @ W^T and |A| @ |W|^T of the stored operands (cached per operand pair)."""
    if key not in _REFS:
        _REFS.clear()
        a, w = A.double(), W.double()
        _REFS[key] = (a @ w.t(), a.abs() @ w.abs().t())
    return _REFS[key]


def gelu64(x):
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def dgelu64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def e_dg(x):
    return torch.where(x.abs() <= 4.5, E_DG_IN, E_DG_OUT) + 8 * U32


# ---- judgment -----------------------------------------------------------------------------------------------------------------
def judge(sec, dt, q, tag, got, ref, gate, tile_gate, skip_rows=()):
    """Per element |got - ref| <= gate; per (row, 256-column tile) and over the whole tensor rel <= tile_gate, except in the rows of
    skip_rows (cancelling rows: their reference is ~0 and only the element gate judges them)."""
    got = got.double()
    err = (got - ref).abs()
    ratio = (err / gate).max().item()
    record(sec, dt, q, ratio, tag)
    bad = err > gate
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag} {q}: {int(bad.sum())} elements outside the gate, first at {i}: got {got[i[0], i[1]].item()!r} "
                             f"ref {ref[i[0], i[1]].item()!r} gate {gate[i[0], i[1]].item():.3e}")
    keep = torch.ones(ref.shape[0], dtype=torch.bool, device=DEV)
    for r in skip_rows:
        keep[r] = False
    e2, r2 = (err * err)[keep], (ref * ref)[keep]
    n = ref.shape[1]
    nt = (n + 255) // 256
    pad = nt * 256 - n
    e2 = torch.nn.functional.pad(e2, (0, pad)).view(-1, nt, 256).sum(-1)
    r2 = torch.nn.functional.pad(r2, (0, pad)).view(-1, nt, 256).sum(-1)
    rel_t = torch.where(r2 > 0, (e2 / r2.clamp_min(1e-300)).sqrt(), torch.where(e2 > 0, math.inf, 0.0))
    worst = rel_t.max().item()
    assert worst <= tile_gate, (tag, q, f"a (row, 256-column tile) has relative error {worst:.3e} > {tile_gate}")
    whole = (e2.sum() / r2.sum().clamp_min(1e-300)).sqrt().item()
    whole_gate = G_T16 if tile_gate == G_T16_2 else tile_gate
    assert whole <= whole_gate, (tag, q, f"whole-tensor relative error {whole:.3e} > {whole_gate}")


# ---- routing (A): mirrors of the host-side decisions of gemm_bf16.hip / gemm_nt_w128.hip ----------------------------------------
def ntw_serves(M, N, Kd):
    return not (Kd % 64 or Kd < 256 or N % 256 or M < 256 or N > 16128)


def ntw_split(M, N, Kd, g):
    """gemm_ntw_split: the 256-row tiles the four-wave launch takes."""
    tiles_n = N // 256
    tm_cap = M // 256 if M % 256 == 0 else (M - 1024) // 256
    if tm_cap <= 0:
        return 0
    second = 14.0 / (0.72 * (Kd // 32) + 6.0)

    def legal(tm):
        rest = M - 256 * tm
        return 0 < tm <= tm_cap and (rest == 0 or rest >= 1024)

    def cost(tm):
        rest = M - 256 * tm
        c = float((tm * tiles_n + g - 1) // g)
        if rest > 0:
            c += second + 0.6 * ((((rest + 127) // 128) * tiles_n + g - 1) // g)
        return c

    best, best_tm = 1e30, 0
    cands = [tm_cap] + ([tm_cap - 4] if M % 256 == 0 and tm_cap > 4 else [])
    k = (tm_cap * tiles_n) // g
    if k >= 1:
        tm = (k * g) // tiles_n
        cands.append(tm)
        while tm > 0 and not legal(tm):
            tm -= 1
        cands.append(tm)
    for tm in cands:
        if legal(tm) and cost(tm) < best:
            best, best_tm = cost(tm), tm
    return best_tm


def fm_of(M, N):
    """nt_plan's tile height (m-fragments) of the 256pp kernel."""
    tn = (N + 255) // 256
    t8, t7 = ((M + 255) // 256) * tn, ((M + 223) // 224) * tn
    return 7 if ((t7 + 255) // 256) * 7 * 10 <= ((t8 + 255) // 256) * 8 * 9 else 8


def route(M, N, Kd, ldc, aux_ok=True):
    """(route name, expected gemm_nt_colsum_rows, four-wave tiles of the full-chip split)"""
    p = K.gemm_nt_plan(M, N, Kd, ldc)
    if not p["persistent"] or not aux_ok:
        if Kd % 32 == 0 and M >= 1024 and N >= 256 and N % 8 == 0 and ldc % 8 == 0 and aux_ok:
            fm = fm_of(M, N)
            return f"256pp-fm{fm}", 2 * ((M + 32 * fm - 1) // (32 * fm)), 0
        return "small", 0, 0
    tmw = ntw_split(M, N, Kd, p["workgroups"]) if ntw_serves(M, N, Kd) else 0
    if tmw == 0:
        return "8-wave", 2 * (p["tiles_m256"] + p["tiles_m128"]), 0
    rest = M - 256 * tmw
    if rest == 0:
        return "4-wave", 2 * tmw, tmw
    q = K.gemm_nt_plan(rest, N, Kd, ldc)
    return "split", 2 * tmw + 2 * (q["tiles_m256"] + q["tiles_m128"]), tmw


# ---- the NT cells ---------------------------------------------------------------------------------------------------------------
EPIS = ["none", "bias", "bias_gelu", "resid", "resid_nobias", "resid16", "gelu_bwd", "dg", "dg8", "mul_aux", "mul_aux8"]
PERSIST_ONLY = {"resid16", "dg", "dg8", "mul_aux", "mul_aux8"}


class Cell:
    """One NT call site: operands, outputs in guarded stores, the float64 references."""

    def __init__(self, M, N, Kd, ldc, dt, seed=1, aux_off=0):
        self.M, self.N, self.Kd, self.ldc, self.dt, self.aux_off = M, N, Kd, ldc, dt, aux_off
        self.A, self.akinds = operand(M, Kd, dt, seed, "a")
        self.W, self.wkinds = operand(N, Kd, dt, seed + 1, "w")
        self.tag = f"{dname(dt)} M={M} N={N} K={Kd} ldc={ldc}" + (f" aux+{aux_off}" if aux_off else "")
        g = torch.Generator(device=DEV)
        g.manual_seed(seed + 7)
        self.bias = (torch.randn(N, generator=g, device=DEV) * 0.5).to(dt)
        self.r32 = Out(M, N, ldc, F32)
        self.r32.v.copy_(torch.randn(M, N, generator=g, device=DEV))
        self.r16 = Out(M, N, ldc, dt)
        self.r16.v.copy_(torch.randn(M, N, generator=g, device=DEV).to(dt))
        self.h = Out(M, N, ldc, dt, off=aux_off)                      # GELU_BWD / MUL_AUX input (16-bit)
        self.h.v.copy_((torch.randn(M, N, generator=g, device=DEV) * 2).to(dt))
        self.h8 = Out(M, N, ldc, torch.uint8, off=2 * aux_off)
        self.h8.v.copy_(torch.arange(M * N, device=DEV).view(M, N).remainder(256).to(torch.uint8))   # all 256 byte values
        self.route, self.R, self.tmw = route(M, N, Kd, ldc, aux_ok=(aux_off % 8 == 0))
        self.ref, self.S = products(self.A, self.W, (M, N, Kd, dt, seed))
        self.e_acc = gamma(Kd) * self.S

    # outputs of one epilogue call: {name: Out}
    def outs(self, epi):
        M, N, ldc, dt = self.M, self.N, self.ldc, self.dt
        o = {"C": Out(M, N, ldc, F32 if epi.startswith("resid") and epi != "resid16" else dt)}
        if epi in ("bias_gelu", "dg"):
            o["aux"] = Out(M, N, ldc, dt, off=self.aux_off)
        if epi == "dg8":
            o["aux"] = Out(M, N, ldc, torch.uint8, off=2 * self.aux_off)
        if epi in ("gelu_bwd", "mul_aux", "mul_aux8") and self.R > 0:
            o["part"] = Out(self.R, N, N, F32)
        return o

    def call(self, epi, o, W=None, ldw=None, drop=None):
        """drop: (p, seed) through vitk_gemm_nt_bf16_drop."""
        A, M, N, Kd, ldc = self.A, self.M, self.N, self.Kd, self.ldc
        W = self.W if W is None else W
        ldw = Kd if ldw is None else ldw
        C = o["C"].v
        aux = o["aux"].v if "aux" in o else None
        part = o["part"].v if "part" in o else None
        E = {"none": L.EPI_NONE, "bias": L.EPI_BIAS, "bias_gelu": L.EPI_BIAS_GELU, "resid": L.EPI_RESID, "resid_nobias": L.EPI_RESID,
             "resid16": L.EPI_RESID16, "gelu_bwd": L.EPI_GELU_BWD, "dg": L.EPI_BIAS_GELU_DG, "dg8": L.EPI_BIAS_GELU_DG8}
        bias = None if epi in ("none", "resid_nobias", "gelu_bwd", "mul_aux", "mul_aux8") else self.bias
        resid = self.r32.v if epi.startswith("resid") and epi != "resid16" else (self.r16.v if epi == "resid16" else None)
        if epi in ("gelu_bwd", "mul_aux", "mul_aux8"):
            aux = self.h8.v if epi == "mul_aux8" else self.h.v
        if drop is not None:
            K.gemm_nt_bf16_drop(A, Kd, W, ldw, C, ldc, M, N, Kd, E[epi], drop[0], drop[1], bias=bias, resid=resid, aux=aux, partials=part)
        elif epi == "gelu_bwd" and part is not None:
            K.gemm_nt_bf16_gelu_bwd_colsum(A, Kd, W, ldw, C, ldc, M, N, Kd, aux, part)
        elif epi == "mul_aux":
            K.gemm_nt_bf16_mul_aux_colsum(A, Kd, W, ldw, C, ldc, M, N, Kd, aux, part)
        elif epi == "mul_aux8":
            K.gemm_nt_bf16_mul_aux8_colsum(A, Kd, W, ldw, C, ldc, M, N, Kd, aux, part)
        else:
            K.gemm_nt_bf16(A, Kd, W, ldw, C, ldc, M, N, Kd, E[epi], bias=bias, resid=resid, aux=aux)

    def served(self, epi):
        if self.route == "small" and epi in PERSIST_ONLY:
            return False
        if self.route.startswith("256pp") and epi in PERSIST_ONLY:
            return False
        return True


def judge_epilogue(sec, cell, epi, o, keep=None, inv=1.0, pre16=None):
    """Per-element gates of every epilogue (keep: the dropout decisions (bool, M x N), inv = 1 / (1 - p))."""
    dt, tag = cell.dt, f"{sec} {cell.tag} [{cell.route}] {epi}"
    u = U16[dt]
    ref, e_acc = cell.ref, cell.e_acc
    C = o["C"].v
    b = cell.bias.double()
    skip = [cell.akinds[k] for k in ("cancel", "near")] if cell.akinds else []
    g16 = G_T16

    def scaled(v, e):
        """dropout on a value v (error e): kept x fl32(1 / (1 - p)) (the factor off by u32 relative, one more rounding), dropped 0"""
        if keep is None:
            return v, e
        vs = v * inv
        es = inv * e + 2 * U32 * inv * (v.abs() + e)
        return torch.where(keep, vs, torch.zeros_like(vs)), torch.where(keep, es, torch.zeros_like(es))

    if epi == "none":
        judge(sec, dt, epi, tag, C, ref, rnd(ref.abs(), e_acc, u) + TINY[dt], g16, skip)
    elif epi in ("bias", "bias_gelu", "dg", "dg8"):
        v = ref + b
        e_pre = rnd(v.abs(), rnd(v.abs(), e_acc, U32), u) + TINY[dt]     # acc + bias in f32, rounded to the 16-bit type
        if epi == "bias":
            judge(sec, dt, epi, tag, C, v, e_pre, g16, skip)
        else:
            if epi == "bias_gelu":
                judge(sec, dt, "pre (aux)", tag, o["aux"].v, v, e_pre, g16, skip)
            # C = fl16(gelu_poly(pre16)): |gelu'| <= 1.13 carries the pre-activation's error, the polynomial adds E_PHI |x|, its f32
            # evaluation (9 fma + the product) at most 16 u32 |x|, then the output rounding
            x = v.abs() + e_pre
            e_g = 1.13 * e_pre + (E_PHI + 16 * U32) * x
            g0 = gelu64(v)
            if keep is not None:            # the dropout scales the ROUNDED gelu in f32 and rounds again
                e_g = rnd(g0.abs(), e_g, u) + TINY[dt]
            gv, eg = scaled(g0, e_g)
            judge(sec, dt, "gelu", tag, C, gv, rnd(gv.abs(), eg, u) + TINY[dt], G_T16_2, skip)
            if epi == "dg":
                # aux = fl16(gelu'_poly(pre16)) against the exact gelu' of the kernel's own pre16 (pre16 from the BIAS_GELU run)
                dg = dgelu64(pre16)
                judge(sec, dt, "gelu' (aux)", tag, o["aux"].v, dg, rnd(dg.abs(), e_dg(pre16), u) + TINY[dt], g16, skip)
    elif epi in ("resid", "resid_nobias", "resid16"):
        v = ref + (b if epi != "resid_nobias" else 0.0)
        e = rnd(v.abs(), e_acc, U32) if epi != "resid_nobias" else e_acc          # acc + bias in f32
        v, e = scaled(v, e)
        r = (cell.r32.v if epi != "resid16" else cell.r16.v).double()
        t = v + r
        e = rnd(t.abs(), e, U32)                                                   # + resid in f32
        if epi == "resid16":
            judge(sec, dt, epi, tag, C, t, rnd(t.abs(), e, u) + TINY[dt], g16, skip)
        else:
            judge(sec, F32, epi, tag, C, t, e + TINY[F32], G_T32, skip)
            if keep is not None:           # dropped elements are the residual exactly
                assert torch.equal(C[~keep], cell.r32.v[~keep]), (tag, "a dropped element is not resid + 0")
    else:                                   # gelu_bwd, mul_aux, mul_aux8: C = fl16(fl16(acc) * factor)
        if epi == "gelu_bwd":
            h = cell.h.v.double()
            fac, efac = dgelu64(h), e_dg(h)
        elif epi == "mul_aux":
            fac, efac = cell.h.v.double(), 0.0
        else:
            fac = (cell.h8.v.double() - 27.0) * 0.005
            efac = 2 * U32 * fac.abs()      # 0.005f is off by u32 relative, one more rounding in the product
        e_a = rnd(ref.abs(), e_acc, u)      # the accumulator rounded to the 16-bit type first
        v = ref * fac
        e = fac.abs() * e_a + (ref.abs() + e_a) * efac
        e = rnd(v.abs(), e, U32)
        v, e = scaled(v, e)
        judge(sec, dt, epi, tag, C, v, rnd(v.abs(), e, u) + TINY[dt], G_T16_2, skip)
    # F: the zero rows of A and the zero rows of W (zero columns of C) give bias / resid / 0 exactly
    if cell.akinds and epi in ("none", "bias", "resid", "resid_nobias", "resid16", "gelu_bwd", "mul_aux", "mul_aux8", "bias_gelu"):
        for kind in ("zero", "zero_last"):
            for sl in ((cell.akinds[kind], slice(None)), (slice(None), cell.wkinds[kind])):
                got = (o["aux"].v if epi == "bias_gelu" else C)[sl]
                if keep is not None and epi != "bias_gelu":
                    continue
                if epi == "none" or epi in ("gelu_bwd", "mul_aux", "mul_aux8"):
                    want = torch.zeros_like(got)
                elif epi in ("bias", "bias_gelu"):
                    want = cell.bias.expand(cell.M, cell.N)[sl]
                elif epi == "resid_nobias":
                    want = cell.r32.v[sl]
                elif epi == "resid":
                    want = (cell.bias.float() + cell.r32.v)[sl]
                else:
                    want = (cell.bias.float() + cell.r16.v.float()).to(dt)[sl]
                assert torch.equal(got.float(), want.float()), (tag, f"{kind} rows of A / W: not exactly bias / resid / 0")


def check_colsum(sec, cell, o, tag, R=None):
    """C: every partial row finite (Out.check), the float64 sum of the rows = the float64 column sum of the kernel's rounded C to
    G_COL of the column's sum |C| (the partial rows are f32 sums of the same rounded values), and vitk_colsum_partials folds them to
    those values.  Returns the fold."""
    R, N = R or cell.R, cell.N
    part = o["part"].v
    C = o["C"].v.double()
    s64 = part.double().sum(0)
    ref = C.sum(0)
    den = C.abs().sum(0)
    err = (s64 - ref).abs()
    ratio = (err / (G_COL * den).clamp_min(1e-300)).max().item()
    record(sec, cell.dt, "colsum partials", ratio, tag)
    assert ratio <= 1, (tag, f"column sums of the partial rows off by {ratio:.2f} of the gate")
    fold = torch.full((N,), float("nan"), device=DEV)
    K.colsum_partials(part, R, N, N, fold)
    ratio = ((fold.double() - ref).abs() / (G_COL * den).clamp_min(1e-300)).max().item()
    record(sec, cell.dt, "colsum fold", ratio, tag)
    assert ratio <= 1, (tag, f"vitk_colsum_partials off by {ratio:.2f} of the gate")
    return fold


def expect_refusal(fn, tag):
    with pytest.raises(L.VitkError):
        fn()


def run_cell(sec, cell, epis=EPIS, switches=True):
    """B (+ C, D, F): every epilogue of `cell` judged, refusals checked, then the switches of D bit-identical."""
    M, N, Kd, ldc, dt = cell.M, cell.N, cell.Kd, cell.ldc, cell.dt
    # A: the route the cell takes
    assert K.gemm_nt_colsum_rows(M, N, Kd, ldc, dt) == cell.R, (cell.tag, cell.route, "column-sum rows (route) differ from the plan")
    for c in RESERVES[1:]:
        set_reserve(c)
        assert K.gemm_nt_colsum_rows(M, N, Kd, ldc, dt) == cell.R, (cell.tag, f"row count changes under reserve {c}")
    set_reserve(0)
    if cell.R == 0:                                   # the small kernel writes no partial rows: the column-sum entry points refuse
        part = torch.zeros(2 * ((M + 127) // 128) * N, device=DEV)      # room for any plan's rows, should one be launched
        C = torch.empty(M, ldc, dtype=dt, device=DEV)
        expect_refusal(lambda: K.gemm_nt_bf16_gelu_bwd_colsum(cell.A, Kd, cell.W, Kd, C, ldc, M, N, Kd, cell.h.v, part), cell.tag)
        expect_refusal(lambda: K.gemm_nt_bf16_mul_aux_colsum(cell.A, Kd, cell.W, Kd, C, ldc, M, N, Kd, cell.h.v, part), cell.tag)
    pre16 = None
    gelu_bits = None
    packed = None
    if cell.route not in ("small",) and not cell.route.startswith("256pp"):
        packed = torch.empty(K.pack_w_nt_bytes(N, Kd) // 2, dtype=dt, device=DEV)
        K.pack_w_nt(cell.W, Kd, N, Kd, packed, None)
    for epi in epis:
        tag = f"{sec} {cell.tag} [{cell.route}] {epi}"
        o = cell.outs(epi)
        if not cell.served(epi):
            for x in o.values():
                x.fill()
            expect_refusal(lambda: cell.call(epi, o), tag)
            for x in o.values():
                assert (bits(x.store) == x.sent).all(), (tag, "a refused call wrote output")
            continue
        if epi == "gelu_bwd" and cell.R == 0 and cell.route != "small":
            raise AssertionError((tag, "no column-sum rows on a route other than the small kernel"))
        base = twice(tag, o, lambda: cell.call(epi, o))
        judge_epilogue(sec, cell, epi, o, pre16=pre16)
        if epi == "bias_gelu":
            pre16 = o["aux"].v.double()
            gelu_bits = bits(o["C"].v).clone()
        if epi in ("dg", "dg8"):
            assert torch.equal(bits(o["C"].v), gelu_bits), (tag, "gelu output differs from BIAS_GELU's")
        if epi == "dg8":
            check_codes(cell, o["aux"].v, pre16, tag)
        fold = check_colsum(sec, cell, o, tag) if "part" in o else None
        if not switches:
            continue
        # D: reserve 32 / 192, the 8-wave kernel alone, the K-blocked W: bit-identical to the default
        variants = [(f"reserve {c}", c, None, False) for c in RESERVES[1:]] + [("VITK_NT_W128=0", 0, "0", False)]
        if packed is not None:
            variants.append(("K-blocked W", 0, None, True))
        for name, c, sw, pk in variants:
            set_reserve(c)
            if sw is not None:
                os.environ["VITK_NT_W128"] = sw
            R8 = cell.R
            part_default = o.get("part")
            try:
                if sw is not None and "part" in o:      # the 8-wave kernel alone writes its own plan's partial rows
                    R8 = K.gemm_nt_colsum_rows(M, N, Kd, ldc, dt)
                    o["part"] = Out(R8, N, N, F32)
                for x in o.values():
                    x.fill()
                if pk:
                    cell.call(epi, o, W=packed, ldw=0)
                else:
                    cell.call(epi, o)
            finally:
                os.environ.pop("VITK_NT_W128", None)
                set_reserve(0)
            for n, x in o.items():
                x.check(f"{tag} {name} {n}")
                if n == "part":
                    if sw is None:
                        f2 = torch.full((N,), float("nan"), device=DEV)
                        K.colsum_partials(x.v, cell.R, N, N, f2)
                        assert torch.equal(f2, fold), (tag, name, "partial rows fold to different column sums")
                    else:
                        check_colsum("D", cell, o, f"{tag} {name}", R=R8)
                        o["part"] = part_default
                    continue
                assert torch.equal(bits(x.store), base[n]), (tag, name, n, "not bit-identical to the default")
        if packed is None and cell.route.startswith("256pp"):
            expect_refusal(lambda: cell.call(epi, o, W=torch.zeros(8, dtype=dt, device=DEV), ldw=0), tag + " K-blocked W")


def check_codes(cell, codes, pre16, tag):
    """DG8 codes = rne(200 gelu'(pre16)) + 27 exactly, where pre16 is the kernel's own 16-bit pre-activation; one off only where
    200 gelu'(pre16) lies within 200 x (the polynomial's error + f32 rounding) of a midpoint."""
    t = 200.0 * dgelu64(pre16) + 27.0
    want = torch.round(t)                                     # half-to-even, like the kernel's magic-number rounding
    d = codes.double() - want
    near = ((t - t.floor() - 0.5).abs() <= 200.0 * (e_dg(pre16) + 4 * U32)) & (d.abs() == 1)
    bad = (d != 0) & ~near
    assert not bad.any(), (tag, f"{int(bad.sum())} DG8 codes differ from rne(200 gelu'(pre)) + 27 away from a midpoint")
    n, tot = MIDPOINTS.get(dname(cell.dt), (0, 0))
    MIDPOINTS[dname(cell.dt)] = (n + int(near.sum()), tot + codes.numel())


# A: (M, N, K, ldc) on both sides of each boundary of gemm_nt_impl / ntp_plan / nt_plan / gemm_ntw_serves
def a_cells(g):
    cells = [
        (1023, 256, 256, 260), (1024, 256, 256, 256),            # M: small kernel / persistent
        (2048, 248, 256, 248), (2048, 256, 256, 256),            # N
        (2048, 260, 256, 260), (2048, 264, 256, 264),            # N % 8 = 4 / 0
        (2048, 256, 256, 260), (2048, 256, 256, 264),            # ldc % 8 = 4 / 0 (ldc > N: guard columns)
        (1024, 16128, 64, 16128), (1792, 16136, 64, 16136), (1024, 16136, 64, 16136),   # ntp_plan's N cap; 256pp fm = 7 / 8
        (4100, 512, 32, 512), (4100, 512, 64, 520), (4100, 512, 96, 512),               # one / two / three K-steps
        (3000, 768, 224, 768), (3000, 768, 256, 768), (3000, 768, 288, 768),            # gemm_ntw_serves at K = 224 / 256 / 288
        (5121, 512, 256, 520), (5247, 512, 256, 512),            # M % 128 = 1 / 127 in the 8-wave tail
        (256 * (g // 2), 512, 256, 512),                         # M % 256 = 0: whole rounds of the four-wave kernel
        (256 * (g // 3 + 1), 768, 3072, 768),                    # the split leaves exactly 1,024 rows
        (256 * (g - 1), 256, 256, 256), (256 * g, 256, 256, 256), (256 * (g + 1), 256, 256, 264),   # one below / at / above a round
    ]
    return cells


def test_routes_cover_every_kernel():
    """A: the cells of test_nt_cell reach every route, with the boundaries the issue of this module lists."""
    g = grid()
    routes = {}
    for M, N, Kd, ldc in a_cells(g):
        r, R, tmw = route(M, N, Kd, ldc)
        routes.setdefault(r, []).append((M, N, Kd, ldc, tmw))
    assert set(routes) == {"small", "256pp-fm7", "256pp-fm8", "8-wave", "split", "4-wave"}, sorted(routes)
    assert route(256 * (g // 3 + 1), 768, 3072, 768)[2] * 256 == 256 * (g // 3 + 1) - 1024
    for d in (-1, 0, 1):
        assert route(256 * (g + d), 256, 256, 256 + 8 * (d > 0))[2] == g + d


@pytest.mark.parametrize("M,N,Kd,ldc", a_cells(256))
def test_nt_cell(M, N, Kd, ldc):
    """A, B, C, D, F for one (M, N, K, ldc) in bfloat16 (the cells that depend on the grid are rebuilt from the device's)."""
    g = grid()
    if g != 256:                                      # the grid-dependent cells follow the device
        i = a_cells(256).index((M, N, Kd, ldc))
        M, N, Kd, ldc = a_cells(g)[i]
    run_cell("AB", Cell(M, N, Kd, ldc, BF))


@pytest.mark.parametrize("epi_aux", ["bias_gelu", "gelu_bwd", "dg", "dg8", "mul_aux", "mul_aux8"])
def test_aux_8_byte_aligned(epi_aux):
    """An aux that is 8- but not 16-byte aligned: the persistent plans refuse it, BIAS_GELU / GELU_BWD run on the small kernel
    (GELU_BWD without column sums), the persistent-only epilogues and the column-sum entry points raise."""
    cell = Cell(2048, 512, 256, 512, BF, aux_off=4)
    assert cell.route == "small" and cell.R == 0
    o = cell.outs(epi_aux)
    if epi_aux in ("bias_gelu", "gelu_bwd"):
        twice(cell.tag, o, lambda: cell.call(epi_aux, o))
        judge_epilogue("AB", cell, epi_aux, o)
    else:
        expect_refusal(lambda: cell.call(epi_aux, o), cell.tag)
    if epi_aux == "gelu_bwd":
        part = torch.zeros(2 * 64 * 512, device=DEV)
        expect_refusal(lambda: K.gemm_nt_bf16_gelu_bwd_colsum(cell.A, 256, cell.W, 256, o["C"].v, 512, 2048, 512, 256, cell.h.v, part),
                       cell.tag)


# E: fused dropout
def e_cells(g):
    # (M, N, K): the split leaves both launches work (GELU_BWD with column sums keeps it under dropout), and a shape where it does not
    return [(256 * (g // 3 + 1), 768, 3072), (5121, 512, 256), (4100, 512, 96)]


@pytest.mark.parametrize("i", range(3))
@pytest.mark.parametrize("p", [0.1, 0.37])
def test_dropout_across_the_row_split(i, p, dt=BF):
    g = grid()
    M, N, Kd = e_cells(g)[i]
    cell = Cell(M, N, Kd, N, dt, seed=11)
    if i < 2:
        assert cell.route == "split" and 0 < cell.tmw * 256 < M, (cell.route, cell.tmw)
    else:
        assert cell.tmw == 0
    seed = 1234 + i
    keep8 = torch.empty(M, N, dtype=torch.uint8, device=DEV)
    K.dropout_keep(keep8, M, N, p, seed)
    keep = keep8.bool()
    inv = 1.0 / (1.0 - p)
    for epi in ("resid", "bias_gelu", "gelu_bwd"):
        tag = f"E p={p} {cell.tag} [{cell.route}] {epi}"
        o = cell.outs(epi)
        twice(tag, o, lambda: cell.call(epi, o, drop=(p, seed)))
        judge_epilogue("E", cell, epi, o, keep=keep, inv=inv)
        if epi == "bias_gelu":
            assert (o["C"].v[~keep] == 0).all(), (tag, "a dropped GELU output is not 0")
        if epi == "gelu_bwd":
            assert (o["C"].v[~keep] == 0).all(), (tag, "a dropped gradient is not 0")
            check_colsum("E", cell, o, tag)
        # p = 0 through _drop: bit-identical to the plain entry
        o0 = cell.outs(epi)
        plain = twice(tag + " plain", o0, lambda: cell.call(epi, o0))
        twice(tag + " p=0", o0, lambda: cell.call(epi, o0, drop=(0.0, seed)))
        for n, x in o0.items():
            if n != "part":
                assert torch.equal(bits(x.store), plain[n]), (tag, n, "p = 0 through _drop differs from the plain entry")


# ---- G: the TN weight gradients -----------------------------------------------------------------------------------------------
class TnCell:
    """dW (N x K) = dY^T X over M rows; dY, X views with guard rows after them (a split that read past its rows would meet them)."""

    def __init__(self, M, N, Kd, dt, seed=21, ldy=None, ldx=None):
        self.M, self.N, self.Kd, self.dt = M, N, Kd, dt
        self.ldy, self.ldx = ldy or N, ldx or Kd
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        self.ys = torch.full(((M + GUARD) * self.ldy,), 1e3, dtype=dt, device=DEV)
        self.xs = torch.full(((M + GUARD) * self.ldx,), 1e3, dtype=dt, device=DEV)
        self.dY = self.ys[:M * self.ldy].view(M, self.ldy)[:, :N]
        self.X = self.xs[:M * self.ldx].view(M, self.ldx)[:, :Kd]
        self.dY.copy_(torch.randn(M, N, generator=g, device=DEV).to(dt))
        self.X.copy_(torch.randn(M, Kd, generator=g, device=DEV).to(dt))
        ek = edge_rows(M) if M >= 64 else {}                 # F: zero, large and cancelling token rows
        if ek:
            self.dY[ek["zero"]] = 0
            self.X[ek["big"]] *= 64
            self.X[ek["cancel"]] = self.X[ek["near"]]
            self.dY[ek["cancel"]] = -self.dY[ek["near"]]
        y, x = self.dY.double(), self.X.double()
        self.ref = y.t() @ x
        self.S = y.abs().t() @ x.abs()
        self.tag = f"{dname(dt)} M={M} N={N} K={Kd}"

    def out(self, odt, ldo):
        return Out(self.N, self.Kd, ldo, odt)

    def judge(self, sec, dw, odt, splits, old=None, tag=""):
        ref = self.ref + (old.double() if old is not None else 0.0)
        e = gamma(self.M + splits) * self.S                   # every summation order of M products + the fold of `splits` slabs
        if old is not None:
            e = rnd(ref.abs(), e, U32)                         # += into dW in f32
        u = U32 if odt == F32 else U16[odt]
        judge(sec, self.dt, f"dW {dname(odt)}", f"{sec} {self.tag} {tag}", dw, ref, rnd(ref.abs(), e, u) + TINY[odt],
              G_T32 if odt == F32 else G_T16)


def prior(N, Kd, odt, seed=5):
    """The values a dW accumulates into."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(N, Kd, generator=g, device=DEV).to(odt)


def tn_run(cell, odt, splits, accumulate=False, ldo=None, sec="G", tag="", old=None):
    ldo = ldo or cell.Kd
    o = cell.out(odt, ldo)
    ws = Out(splits, cell.N * cell.Kd, cell.N * cell.Kd, F32)
    if not accumulate:
        old = None
    elif old is None:
        old = prior(cell.N, cell.Kd, odt)

    def call():
        if accumulate:
            o.v.copy_(old)
        K.gemm_tn_bf16(cell.dY, cell.ldy, cell.X, cell.ldx, o.v, ldo, cell.M, cell.N, cell.Kd, ws.v, splits, accumulate=accumulate)

    tg = f"{tag} splits={splits} odt={dname(odt)} acc={int(accumulate)} ldo={ldo}"
    snap = twice(f"{sec} {cell.tag} {tg}", {"dW": o, "ws": ws}, call)
    cell.judge(sec, o.v, odt, splits, old, tg)
    return snap["dW"]


def tn_large(M, N, Kd):
    return M >= 4096 and N >= 256 and Kd >= 256


TN_SHAPES = [(4095, 256, 256), (4096, 256, 256), (4096, 248, 256), (4096, 256, 248),      # tn_large boundaries
             (4100, 264, 520), (4096, 520, 264), (1000, 8, 24), (4100, 24, 8)]             # N, K off multiples of 128 / 256


@pytest.mark.parametrize("M,N,Kd", TN_SHAPES)
@pytest.mark.parametrize("odt", [F32, BF])
def test_tn_shapes(M, N, Kd, odt):
    cell = TnCell(M, N, Kd, BF)
    s = K.gemm_tn_splits(M, N, Kd)
    tn_run(cell, odt, s, tag="planner")
    tn_run(cell, odt, s, accumulate=True, ldo=Kd + 8, tag="planner")


def test_tn_planner_splits_under_reserve():
    cell = TnCell(8192, 768, 768, BF)
    seen = set()
    try:
        for c in RESERVES:
            set_reserve(c)
            s = K.gemm_tn_splits(8192, 768, 768)
            seen.add(s)
            tn_run(cell, F32, s, tag=f"reserve {c}")
    finally:
        set_reserve(0)
    assert len(seen) > 1, "the reserve does not change the planner's split count"


@pytest.mark.parametrize("M,splits", [(4096, 1), (4100, 3), (4128, 64), (4128, 7), (6000, 5)])
def test_tn_caller_splits(M, splits):
    """splits of 1, splits whose last one ends inside a 32-row step (4100 / 3: 1,348 rows), splits whose last ones hold no rows
    (4128 / 64: 96 rows each, 43 splits), odd step counts (the kernel runs a step past a split's end on a zero-filled stage)."""
    cell = TnCell(M, 512, 256, BF)
    tn_run(cell, F32, splits)
    tn_run(cell, BF, splits, accumulate=True, ldo=264)


def test_tn_row_stride_beyond_the_four_wave_kernel():
    """A row stride with (rows of a split + 160) x ldy x 2 >= 2^31: gemm_tn_w128_serves refuses it and the 128 x 128 kernel serves
    the large shape.  One 2 GiB buffer holds dY (columns 0..255) and X (columns 256..511)."""
    M, N, Kd, ld = 4096, 256, 256, 1 << 18
    assert (M + 160) * ld * 2 >= 1 << 31
    buf = torch.empty(M + 1, ld, dtype=BF, device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    buf[:, :512] = torch.randn(M + 1, 512, generator=g, device=DEV).to(BF)
    dY, X = buf[:M, :N], buf[:M, 256:256 + Kd]
    ref = dY.double().t() @ X.double()
    S = dY.double().abs().t() @ X.double().abs()
    dW = Out(N, Kd, Kd, F32)
    ws = Out(1, N * Kd, N * Kd, F32)
    twice("G ldy 2^18", {"dW": dW, "ws": ws}, lambda: K.gemm_tn_bf16(dY, ld, X, ld, dW.v, Kd, M, N, Kd, ws.v, 1))
    judge("G", BF, "dW f32 (128 x 128 kernel, ldy 2^18)", "G ldy=2^18", dW.v, ref, rnd(ref.abs(), gamma(M + 1) * S, U32) + TINY[F32], G_T32)
    del buf


PAIR_SHAPES = [(4095, 768, 768, 256, 256), (4096, 768, 768, 248, 256), (4096, 768, 768, 256, 248), (4096, 768, 768, 256, 256)]


@pytest.mark.parametrize("M,N0,K0,N1,K1", PAIR_SHAPES)
def test_tn_pair_boundaries(M, N0, K0, N1, K1):
    s = K.gemm_tn_pair_splits(M, N0, K0, N1, K1)
    served = tn_large(M, N0, K0) and tn_large(M, N1, K1)
    assert (s > 0) == served, (M, N1, K1, s)
    c0, c1 = TnCell(M, N0, K0, BF, seed=31), TnCell(M, N1, K1, BF, seed=32)
    if not served:
        dW0, dW1 = torch.empty(N0, K0, device=DEV), torch.empty(N1, K1, device=DEV)
        ws = torch.empty(N0 * K0 + N1 * K1, device=DEV)
        expect_refusal(lambda: K.gemm_tn_bf16_pair(c0.dY, N0, c0.X, K0, dW0, c1.dY, N1, c1.X, K1, dW1, M, ws, 1), "pair")
        return
    pair_run(c0, c1, F32, BF, acc0=False, acc1=True)
    os.environ["VITK_TN_PAIR"] = "0"
    try:
        assert K.gemm_tn_pair_splits(M, N0, K0, N1, K1) == 0
    finally:
        os.environ.pop("VITK_TN_PAIR", None)


def pair_run(c0, c1, odt, dt, acc0, acc1, tag=""):
    """The pair (dW0 with ldo0 = K0 + 8 guard columns) judged per element, bit-identical to two single launches with its split count."""
    M, N0, K0, N1, K1 = c0.M, c0.N, c0.Kd, c1.N, c1.Kd
    s = K.gemm_tn_pair_splits(M, N0, K0, N1, K1, dt)
    assert s > 0
    o0, o1 = c0.out(odt, K0 + 8), c1.out(odt, K1)
    ws = Out(s, N0 * K0 + N1 * K1, N0 * K0 + N1 * K1, F32)
    old0, old1 = prior(N0, K0, odt, 9), prior(N1, K1, odt, 10)
    lib = L.load_f16() if dt == F16 else L.load()

    def call():             # (the wrapper in kernels.py takes ldo = K; the C entry point takes any ldo)
        if acc0:
            o0.v.copy_(old0)
        if acc1:
            o1.v.copy_(old1)
        L.check(lib.vitk_gemm_tn_bf16_pair(c0.dY.data_ptr(), N0, c0.X.data_ptr(), K0, o0.v.data_ptr(), K0 + 8, int(acc0), N0, K0,
                                           c1.dY.data_ptr(), N1, c1.X.data_ptr(), K1, o1.v.data_ptr(), K1, int(acc1), N1, K1,
                                           K.dt(odt), M, ws.v.data_ptr(), s, torch.cuda.current_stream().cuda_stream), "gemm_tn_bf16_pair")

    pair = twice(f"G pair {c0.tag} {c1.tag} {tag}", {"dW0": o0, "dW1": o1, "ws": ws}, call)
    c0.judge("G", o0.v, odt, s, old0 if acc0 else None, f"pair {tag} acc={int(acc0)}")
    c1.judge("G", o1.v, odt, s, old1 if acc1 else None, f"pair {tag} acc={int(acc1)}")
    a = tn_run(c0, odt, s, accumulate=acc0, ldo=K0 + 8, tag="single", old=old0)
    b = tn_run(c1, odt, s, accumulate=acc1, tag="single", old=old1)
    assert torch.equal(pair["dW0"], a) and torch.equal(pair["dW1"], b), (tag, "the pair differs from two single launches")
    return s


@pytest.mark.parametrize("reserve", [0, 32])
@pytest.mark.parametrize("odt", [F32, BF])
def test_tn_pair_against_two_launches(reserve, odt, dt=BF):
    M, N0, K0, N1, K1 = 8192, 2304, 768, 768, 768
    c0, c1 = TnCell(M, N0, K0, dt, seed=41), TnCell(M, N1, K1, dt, seed=42)
    try:
        s0 = K.gemm_tn_pair_splits(M, N0, K0, N1, K1, dt)
        set_reserve(reserve)
        s = pair_run(c0, c1, odt, dt, acc0=True, acc1=False, tag=f"reserve {reserve}")
        assert (s != s0) == (reserve > 0), ("the reserve should change the pair's split count here", s0, s)
    finally:
        set_reserve(0)


# ---- H: the IEEE-half library ----------------------------------------------------------------------------------------------------
H_NT = [(1023, 256, 256, 256), (2048, 264, 256, 264), (1792, 16136, 64, 16136), (5121, 512, 256, 512), (3000, 768, 256, 768)]


@pytest.mark.parametrize("M,N,Kd,ldc", H_NT)
def test_half_nt_cell(M, N, Kd, ldc):
    run_cell("H", Cell(M, N, Kd, ldc, F16, seed=51))


@pytest.mark.parametrize("p", [0.25])
def test_half_dropout(p):
    test_dropout_across_the_row_split(1, p, dt=F16)


@pytest.mark.parametrize("M,N,Kd,splits", [(4128, 512, 256, 64), (4095, 256, 256, 0), (4100, 264, 520, 0)])
def test_half_tn(M, N, Kd, splits):
    cell = TnCell(M, N, Kd, F16, seed=61)
    s = splits or K.gemm_tn_splits(M, N, Kd, F16)
    tn_run(cell, F32, s, sec="H")
    tn_run(cell, F16, s, accumulate=True, ldo=Kd + 8, sec="H")


def test_half_tn_pair():
    test_tn_pair_against_two_launches(32, F16, dt=F16)
