"""GPU: the 16-bit attention kernels at every dispatch boundary, against float64, judged per (batch, head) item.

Which kernel serves a call depends on N, dim_head, the dropout probability and VITK_ATTN_PIPE / VITK_ATTN_R_* (attention.hip
vitk_attn_*_bf16_drop, attention_pipe.hip attn_pipe_supported / attn_fused_bwd_supported, ops.attn_fwd / attn_bwd).  The cells
here sit on both sides of every range limit (32/33, 128/129, 192/193, 208/209, 224/225, 256/257, 480) under every switch setting;
a setting that does not apply at some N falls back to the per-head kernels, so the cells stay meaningful when the ranges move.

 A. fixed-length matrix (dim_head 64), and item counts one past a full round of the persistent grids;
 B. dropout on the attention matrix, including the pipelined forward / dK-dV kernels and the fused backward's bypass;
 C. awkward score values: all far below / far above zero, a late maximum jump just under / over the lazy-maximum threshold
    (2^8 in the exp2 domain), constant rows, scales other than d^-0.5;
 D. padded and separate-tensor layouts, with sentinel guards around every output and input slice;
 E. the dense shapes the variable-length kernels serve (ops.attn_fwd / attn_bwd), up to BASELINE config 5's extents.

Every cell: outputs pre-filled with NaN (a tile that is never written fails), everything finite, each (b, h) item held to the
whole-tensor gates of test_kernels_gpu.py / test_attention_pipe_gpu.py on its own (a wrong ragged tile of one head, or a race
in a persistent kernel's buffer hand-over that damages a few rows of one item, fails here), the whole tensor too, and two
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
LOG2E = 1.4426950408889634

SWITCHES = ("VITK_ATTN_PIPE", "VITK_ATTN_R_FWD", "VITK_ATTN_R_DQ", "VITK_ATTN_R_DKV")
_R = ("VITK_ATTN_R_FWD", "VITK_ATTN_R_DQ", "VITK_ATTN_R_DKV")
SETTINGS = {
    "default": {},
    "per_head": {"VITK_ATTN_PIPE": "0"},
    "pipelined": {"VITK_ATTN_PIPE": "7"},
    "pipelined_fused": {"VITK_ATTN_PIPE": "15"},
    "per_head_r1": {"VITK_ATTN_PIPE": "0", **{v: "1" for v in _R}},
    "per_head_r2": {"VITK_ATTN_PIPE": "0", **{v: "2" for v in _R}},
}
PIPE_SETTINGS = ("default", "per_head", "pipelined", "pipelined_fused")

# Per-item gates = the existing whole-tensor gates: (o, dq / dk / dv relative L2, lse max abs)
GATES = {BF: (6e-3, 1.2e-2, 4e-3), F16: (1e-3, 2e-3, 4e-3)}
DROP_GATES = (8e-3, 1.5e-2, 4e-3)
# dq and dk of an item can vanish (N = 1; constant rows make dq exactly zero): their error is then measured against
# FLOOR x ||dv_ref|| of the same item instead of their own norm -- an absolute error on the scale of the item's gradients
FLOOR = 0.05
# delta = rowsum(dO * O) is summed in f32 from 16-bit products (exact in f32): 1e-4 of the row's sum of |dO * O| is generous
DELTA_TOL = 1e-4

SENTINEL16 = 0x7FA5             # NaN bit patterns no kernel writes (positive as int16 / int32)
SENTINEL32 = 0x7FBADBAD


def use(monkeypatch, setting):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)


def fused_may_run(setting, N, d=64, p=0.0):
    """The single-kernel backward keeps delta in LDS: the delta buffer is scratch there (include/vitk.h), so it is judged only
    where the two-kernel path runs.  Mirrors attn_fused_bwd_supported() for the settings that enable it."""
    return setting in ("default", "pipelined_fused") and d == 64 and 192 < N <= 208 and p == 0.0


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def randn(shape, g, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


# ---- float64 reference and the per-item judge -----------------------------------------------------------------------
def reference(q, k, v, do, scale, keep=None, o_kernel=None):
    """softmax(scale q k^T) v and its backward in float64 from the exact 16-bit inputs; (G, N, d) each.  keep: (G, N, N) mask
    already scaled by 1 / (1 - p) (nn.Dropout on the probabilities; lse and the softmax denominators are the undropped ones).
    o_kernel: the kernel's own (16-bit) o -- the backward's delta = rowsum(dO * O) is then built from it, as every flash backward
    does; with the exact o instead, the 16-bit rounding of o alone moves dq / dk by percents wherever one key dominates a row
    (dP - delta cancels)."""
    q, k, v, do = (t.to(F64) for t in (q, k, v, do))
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    pk = p if keep is None else p * keep
    o = pk @ v
    dv = pk.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    if keep is not None:
        dp = dp * keep
    ds = p * (dp - (do * (o if o_kernel is None else o_kernel.to(F64))).sum(-1)[..., None])
    dq = (ds @ k) * scale
    dk = (ds.transpose(-1, -2) @ q) * scale
    return o, lse, dq, dk, dv


def judge(tag, ins, outs, scale, gates, keep_fn=None, judge_delta=True, chunk=None):
    """ins: q, k, v, do as (B, H, N, d) views of the 16-bit inputs; outs: o, dq, dk, dv (B, H, N, d), lse, delta (B, H, N).
    Reference work is chunked over batch entries.  Asserts on the WORST (b, h) item and on the whole tensor."""
    B, H, N, d = ins["q"].shape
    for name in ("o", "dq", "dk", "dv", "lse") + (("delta",) if judge_delta else ()):
        assert torch.isfinite(outs[name].float()).all(), (tag, name, "non-finite (unwritten or overflowed) entries")
    if chunk is None:
        chunk = max(1, min(B, (1 << 24) // max(1, H * N * N)))
    worst = {n: (0.0, None) for n in ("o", "dq", "dk", "dv", "lse", "delta")}
    sq = {n: [0.0, 0.0] for n in ("o", "dq", "dk", "dv")}
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        G = (b1 - b0) * H
        flat = lambda t: t[b0:b1].reshape(G, *t.shape[2:])
        keep = keep_fn(b0, b1) if keep_fn else None
        ko = flat(outs["o"])
        ro, rl, rdq, rdk, rdv = reference(flat(ins["q"]), flat(ins["k"]), flat(ins["v"]), flat(ins["do"]), scale, keep, ko)
        dvn = rdv.flatten(1).norm(dim=1)
        for name, ref in (("o", ro), ("dq", rdq), ("dk", rdk), ("dv", rdv)):
            x = flat(outs[name]).to(F64)
            e = (x - ref).flatten(1).norm(dim=1)
            n = ref.flatten(1).norm(dim=1)
            den = torch.maximum(n, FLOOR * dvn) if name in ("dq", "dk") else n
            sq[name][0] += (e * e).sum().item()
            sq[name][1] += (den * den).sum().item()
            r = e / den.clamp_min(1e-30)
            i = int(r.argmax())
            if r[i].item() > worst[name][0] or worst[name][1] is None:
                worst[name] = (r[i].item(), divmod(b0 * H + i, H))
        el = (flat(outs["lse"]).to(F64) - rl).abs().amax(1)
        i = int(el.argmax())
        if el[i].item() >= worst["lse"][0]:
            worst["lse"] = (el[i].item(), divmod(b0 * H + i, H))
        if judge_delta:
            prod = flat(ins["do"]).to(F64) * ko.to(F64)         # delta is rowsum(dO * O) of the kernel's OWN o
            ed = ((flat(outs["delta"]).to(F64) - prod.sum(-1)).abs() / (prod.abs().sum(-1) + 1e-6)).amax(1)
            i = int(ed.argmax())
            if ed[i].item() >= worst["delta"][0]:
                worst["delta"] = (ed[i].item(), divmod(b0 * H + i, H))
    whole = {n: math.sqrt(s[0]) / max(math.sqrt(s[1]), 1e-30) for n, s in sq.items()}
    print(f"[attn-judge] {tag}: worst item " + " ".join(f"{n} {v:.2e}@{it}" for n, (v, it) in worst.items())
          + " | whole " + " ".join(f"{n} {v:.2e}" for n, v in whole.items()))
    go, gg, gl = gates
    for n in ("o", "dq", "dk", "dv"):
        gate = go if n == "o" else gg
        assert worst[n][0] < gate, (tag, n, "worst (b, h) item", worst[n], gate)
        assert whole[n] < gate, (tag, n, "whole tensor", whole[n], gate)
    assert worst["lse"][0] < gl, (tag, "lse", worst["lse"], gl)
    if judge_delta:
        assert worst["delta"][0] < DELTA_TOL, (tag, "delta", worst["delta"], DELTA_TOL)
    return worst


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_same_bits(tag, a, b, names):
    for n in names:
        assert torch.equal(bits(a[n]), bits(b[n])), (tag, n, "differs between two identical runs")


# ---- fixed-length calls (vitk_attn_{fwd,bwd}_bf16_drop) in several layouts ----------------------------------------------
class Operand:
    """A (B, H, N, d) operand inside a flat storage: element strides (s_b, s_h, s_n), contiguous columns."""

    def __init__(self, store, off, s_b, s_h, s_n, shape):
        self.store, self.off, self.s = store, off, (s_b, s_h, s_n)
        self.shape = shape

    def view(self):
        return self.store.as_strided(self.shape, (*self.s, 1), self.off)

    def desc(self):
        return K.bhnd(self.store, *self.s, offset=self.off)


class Layout:
    """Inputs q, k, v, dO and outputs o, dq, dk, dv of one fixed-length call.
    dense:    the merged (B, N, 3 I) to_qkv layout the engine uses (s_n = 3 I), o / dO (B, N, I);
    padded:   the merged layouts with 64 (qkv, dqkv) / 32 (o, dO) padding elements per row;
    separate: six tensors q, k, v, dq, dk, dv with their own head / row / batch strides (multiples of 8, gaps everywhere).
    Outside dense, every storage holds at least one whole item past the last real one; everything that is not a real element
    (padding columns, gaps, the guard item) holds a sentinel bit pattern that must survive the call bit for bit.  lse and delta
    always carry a guard tail of one batch entry + 64 floats."""

    def __init__(self, kind, B, H, N, d, dtype):
        self.B, self.H, self.N, self.d, self.dtype, self.kind = B, H, N, d, dtype, kind
        I = H * d
        shape = (B, H, N, d)
        self.stores = []

        def store(numel):
            t = torch.empty(numel, dtype=dtype, device=DEV)
            bits(t).fill_(SENTINEL16)
            self.stores.append(t)
            return t

        def merged(n_terms, pad):
            s_n = n_terms * I + pad
            s_b = N * s_n
            st = store(s_b * (B + (1 if kind != "dense" else 0)))
            return [Operand(st, t * I, s_b, d, s_n, shape) for t in range(n_terms)]

        if kind == "dense":
            self.q, self.k, self.v = merged(3, 0)
            self.dq, self.dk, self.dv = merged(3, 0)
            (self.o,), (self.do,) = merged(1, 0), merged(1, 0)
        elif kind == "padded":
            self.q, self.k, self.v = merged(3, 64)
            self.dq, self.dk, self.dv = merged(3, 64)
            (self.o,), (self.do,) = merged(1, 32), merged(1, 32)
        else:
            ops_ = []
            for j in range(6):
                s_h = d + 8 * (j % 3)
                s_n = H * s_h + 8 * (j + 1)
                s_b = (N + j % 2) * s_n
                ops_.append(Operand(store(s_b * (B + 1)), 8 * j, s_b, s_h, s_n, shape))
            self.q, self.k, self.v, self.dq, self.dk, self.dv = ops_
            (self.o,), (self.do,) = merged(1, 32), merged(1, 32)
        tail = H * N + 64
        self.lse = torch.empty(B * H * N + tail, dtype=F32, device=DEV)
        self.delta = torch.empty_like(self.lse)
        for t in (self.lse, self.delta):
            t.view(torch.int32).fill_(SENTINEL32)
        # real-element masks of every storage (guards = the complement)
        self.real = []
        for st in self.stores:
            m = torch.zeros(st.numel(), dtype=torch.bool, device=DEV)
            for opd in self.operands():
                if opd.store is st:
                    m.as_strided(shape, (*opd.s, 1), opd.off).fill_(True)
            self.real.append(m)
        self.n_real = B * H * N

    def operands(self):
        return (self.q, self.k, self.v, self.do, self.o, self.dq, self.dk, self.dv)

    def load(self, q, k, v, do):
        for opd, x in ((self.q, q), (self.k, k), (self.v, v), (self.do, do)):
            opd.view().copy_(x.to(self.dtype))

    def ins(self):
        return {"q": self.q.view(), "k": self.k.view(), "v": self.v.view(), "do": self.do.view()}

    def clear(self):
        for opd in (self.o, self.dq, self.dk, self.dv):
            opd.view().fill_(float("nan"))
        self.lse[:self.n_real].fill_(float("nan"))
        self.delta[:self.n_real].fill_(float("nan"))

    def run(self, scale, p=0.0, seed=0):
        B, H, N, d = self.B, self.H, self.N, self.d
        self.clear()
        K.attn_fwd_bf16(self.q.desc(), self.k.desc(), self.v.desc(), self.o.desc(), self.lse, B, H, N, d, scale, p, seed)
        K.attn_bwd_bf16(self.q.desc(), self.k.desc(), self.v.desc(), self.o.desc(), self.do.desc(), self.lse, self.delta,
                        self.dq.desc(), self.dk.desc(), self.dv.desc(), B, H, N, d, scale, p, seed)
        return self.outs()

    def outs(self):
        r = {n: getattr(self, n).view().clone() for n in ("o", "dq", "dk", "dv")}
        r["lse"] = self.lse[:self.n_real].view(self.B, self.H, self.N).clone()
        r["delta"] = self.delta[:self.n_real].view(self.B, self.H, self.N).clone()
        return r

    def assert_guards(self, tag):
        for i, (st, m) in enumerate(zip(self.stores, self.real)):
            g = bits(st)[~m]
            assert (g == SENTINEL16).all(), (tag, f"storage {i}: {(g != SENTINEL16).sum().item()} guard elements changed")
        for name, t in (("lse", self.lse), ("delta", self.delta)):
            assert (t[self.n_real:].view(torch.int32) == SENTINEL32).all(), (tag, name, "guard tail changed")


def keep_mask(B, H, N, p, seed):
    """(b0, b1) -> the float64 keep mask / (1 - p) the fused dropout kernels apply to those batch entries."""
    keep = torch.empty(B * H * N, N, dtype=torch.uint8, device=DEV)
    K.dropout_keep(keep, B * H * N, N, p, seed)
    keep = keep.view(B, H, N, N)
    return lambda b0, b1: keep[b0:b1].reshape(-1, N, N).to(F64) / (1 - p)


def check_fixed(tag, setting, lay, q, k, v, do, scale, gates, p=0.0, seed=0, guards=False):
    lay.load(q, k, v, do)
    out = lay.run(scale, p, seed)
    jd = not fused_may_run(setting, lay.N, lay.d, p)
    keep_fn = keep_mask(lay.B, lay.H, lay.N, p, seed) if p > 0 else None
    worst = judge(tag, lay.ins(), out, scale, gates, keep_fn, judge_delta=jd)
    if guards:
        lay.assert_guards(tag)
    out2 = lay.run(scale, p, seed)                      # run-to-run bit identity: a race in a buffer hand-over shows up here
    assert_same_bits(tag, out, out2, ("o", "lse", "dq", "dk", "dv") + (("delta",) if jd else ()))
    if guards:
        lay.assert_guards(tag)
    return out, worst


def random_inputs(B, H, N, d, seed, scale=1.5):
    g = gen(seed)
    shape = (B, H, N, d)
    return randn(shape, g, scale), randn(shape, g, scale), randn(shape, g, scale), randn(shape, g)


# ---- A. fixed-length matrix ------------------------------------------------------------------------------------------
NS_A = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 127, 128, 129, 160, 191, 192, 193, 196, 197, 207, 208, 209, 223, 224, 225,
        255, 256, 257, 288, 300, 385, 449, 479, 480]
CELLS_A = [(s, BF) for s in SETTINGS] + [("default", F16), ("per_head", F16)]


@pytest.mark.parametrize("N", NS_A)
@pytest.mark.parametrize("setting,dtype", CELLS_A, ids=[f"{s}-{str(t)[6:]}" for s, t in CELLS_A])
def test_fixed_length_matrix(N, setting, dtype, monkeypatch):
    use(monkeypatch, setting)
    B, H, d = 2, 3, 64
    lay = Layout("dense", B, H, N, d, dtype)
    check_fixed(f"A N={N} {setting} {dtype}", setting, lay, *random_inputs(B, H, N, d, 1000 + N), d ** -0.5, GATES[dtype])


@pytest.mark.parametrize("N", [33, 129, 197, 208, 224])
@pytest.mark.parametrize("setting", ["default", "pipelined", "pipelined_fused"])
@pytest.mark.parametrize("rounds", [1, 2])
def test_items_one_past_the_persistent_grid(N, setting, rounds, monkeypatch):
    """B*H = rounds * CUs + 1: one item past a full round of the backward grid (one workgroup per CU) and of the forward grid
    (two per CU) -- the last item is the only one of its round and inherits buffers from the previous one."""
    use(monkeypatch, setting)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, H, d = rounds * cus + 1, 1, 64
    lay = Layout("dense", B, H, N, d, BF)
    check_fixed(f"A-grid N={N} {setting} items={B}", setting, lay, *random_inputs(B, H, N, d, 2000 + N), d ** -0.5, GATES[BF])


# ---- B. dropout --------------------------------------------------------------------------------------------------------
NS_B = [17, 33, 64, 129, 197, 208, 224, 257, 480]


@pytest.mark.parametrize("N", NS_B)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("setting", ["default", "per_head_r1", "per_head_r2", "pipelined"])
def test_dropout_against_float64(N, p, setting, monkeypatch):
    """nn.Dropout on the attention matrix (the *_bf16_drop entries) against float64 with the very same keep decisions; same seed
    bit-identical (check_fixed), another seed a different o.  `pipelined` runs attn_fwd_pipe_kernel<1, true> and the pipelined
    dK/dV kernel with dropout; at N = 197 / 208 `default` checks that dropout bypasses the fused backward."""
    use(monkeypatch, setting)
    B, H, d, seed = 2, 3, 64, 4321 + N
    lay = Layout("dense", B, H, N, d, BF)
    out, _ = check_fixed(f"B N={N} p={p} {setting}", setting, lay, *random_inputs(B, H, N, d, 3000 + N), d ** -0.5, DROP_GATES,
                         p=p, seed=seed)
    other = lay.run(d ** -0.5, p, seed + 1)
    assert (bits(other["o"]) != bits(out["o"])).float().mean().item() > 0.5, "another seed must drop other entries"


@pytest.mark.parametrize("N", NS_B)
@pytest.mark.parametrize("setting", ["default", "per_head_r1", "per_head_r2", "pipelined", "pipelined_fused"])
def test_dropout_p0_equals_plain_entry(N, setting, monkeypatch):
    """p = 0 through the _drop entries is the plain entry, bit for bit (same kernels, no dropout template)."""
    use(monkeypatch, setting)
    B, H, d = 2, 3, 64
    scale = d ** -0.5
    lay = Layout("dense", B, H, N, d, BF)
    lay.load(*random_inputs(B, H, N, d, 3500 + N))
    a = lay.run(scale, 0.0, 99)
    lay.clear()
    lib = L.load()
    L.check(lib.vitk_attn_fwd_bf16(lay.q.desc(), lay.k.desc(), lay.v.desc(), lay.o.desc(), K._p(lay.lse), B, H, N, d, scale,
                                   K._stream()), "attn_fwd_bf16")
    L.check(lib.vitk_attn_bwd_bf16(lay.q.desc(), lay.k.desc(), lay.v.desc(), lay.o.desc(), lay.do.desc(), K._p(lay.lse),
                                   K._p(lay.delta), lay.dq.desc(), lay.dk.desc(), lay.dv.desc(), B, H, N, d, scale, K._stream()),
            "attn_bwd_bf16")
    b = lay.outs()
    assert_same_bits(f"B p=0 N={N} {setting}", a, b, ("o", "lse", "dq", "dk", "dv"))


# ---- C. score edge values ------------------------------------------------------------------------------------------------
def edge_inputs(case, B, H, N, d, seed):
    """q, k, v, dO (float32, cast by the caller) and the scale.  Scores in exp2 units are (q . k) * scale * log2(e)."""
    g = gen(seed)
    shape = (B, H, N, d)
    v, do = randn(shape, g, 1.5), randn(shape, g)
    scale = d ** -0.5
    c = scale * LOG2E
    if case in ("far_below", "far_above"):
        # score = q0 * 4 + (63 random dims: std ~1.4 exp2 units); the per-row offset q0 * 4 * c lies in [-54, -46] / [200, 300]:
        # real scores far from zero but not uniform, so an unmasked zero-score padding key would dominate a far_below row
        lo, hi = (-54.0, -46.0) if case == "far_below" else (200.0, 300.0)
        q, k = randn(shape, g), randn(shape, g)
        q[..., 0] = (lo + (hi - lo) * torch.rand(B, H, N, generator=g, device=DEV)) / (4.0 * c)
        k[..., 0] = 4.0
        return q, k, v, do, scale
    if case.startswith("jump"):
        # every key but the special ones scores -u_j (u_j in [0, 3) exp2 units, 0 at every 16th key so each key fragment
        # holds the row maximum exactly); the special key's score exceeds the running maximum by 43 c = 7.75 / 45.5 c = 8.21
        # exp2 units (raw margins exact in bf16 and half, also on top of 32): the lazy branch with P up to 2^7.75 / the
        # rescale branch
        _, place, sign = case.split("_")
        margin = 43.0 if sign == "minus" else 45.5
        q = randn(shape, g)
        q[..., 0] = 1.0
        q[..., 2] = 1.0
        k = torch.zeros(shape, device=DEV)
        u = torch.rand(B, H, N, generator=g, device=DEV) * (3.0 / c)
        u[..., ::16] = 0.0
        k[..., 2] = -u
        k[..., N - 1, 2] = 0.0
        if place == "last":                              # in the last key step, at key N - 1
            k[..., N - 1, 0] = margin
        else:                                            # key 1 (first step) raises the maximum to 32 c, key N - 1 jumps from there
            k[..., 1, 2] = 0.0
            k[..., 1, 0] = 32.0
            k[..., N - 1, 0] = 32.0 + margin
        return q, k, v, do, scale
    if case == "constant":                              # every key of an item identical: exactly uniform rows
        q = randn(shape, g, 1.5)
        k = randn((B, H, 1, d), g, 0.125).expand(shape).contiguous()
        return q, k, v, do, scale
    if case == "scale_1":
        return randn(shape, g, 0.5), randn(shape, g, 0.5), v, do, 1.0
    if case == "scale_0.02":
        return randn(shape, g, 1.5), randn(shape, g, 1.5), v, do, 0.02
    raise ValueError(case)


CASES_C = ["far_below", "far_above", "jump_last_minus", "jump_last_plus", "jump_first_minus", "jump_first_plus", "constant",
           "scale_1", "scale_0.02"]


@pytest.mark.parametrize("case", CASES_C)
@pytest.mark.parametrize("N", [17, 64, 197, 208, 257, 480])
@pytest.mark.parametrize("setting", PIPE_SETTINGS)
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
def test_score_edge_values(case, N, setting, dtype, monkeypatch):
    use(monkeypatch, setting)
    B, H, d = 2, 2, 64
    q, k, v, do, scale = edge_inputs(case, B, H, N, d, 4000 + N)
    lay = Layout("dense", B, H, N, d, dtype)
    lay.load(q, k, v, do)
    if case.startswith("jump"):                          # the construction survives the 16-bit rounding: margin on the right side of 8
        s2 = (lay.q.view().to(F64) @ lay.k.view().to(F64).transpose(-1, -2)) * scale * LOG2E
        m = s2[..., N - 1] - s2[..., :N - 1].amax(-1)
        lo, hi = (7.7, 7.8) if case.endswith("minus") else (8.15, 8.3)
        assert lo < m.min().item() and m.max().item() < hi, (case, m.min().item(), m.max().item())
    check_fixed(f"C {case} N={N} {setting} {dtype}", setting, lay, q, k, v, do, scale, GATES[dtype])


# ---- D. layouts and output guards ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["padded", "separate"])
@pytest.mark.parametrize("N", [17, 197, 208, 257, 480])
@pytest.mark.parametrize("setting", PIPE_SETTINGS)
def test_layouts_and_guards(kind, N, setting, monkeypatch):
    """Padded row strides, separate tensors with their own strides, and a guard item past the last real one: every padding
    column, gap and guard (inputs included) and the lse / delta guard tails keep their sentinel bits through forward and
    backward -- a store outside an item's (b, h) slice changes a sentinel, never faults."""
    use(monkeypatch, setting)
    B, H, d = 2, 3, 64
    lay = Layout(kind, B, H, N, d, BF)
    check_fixed(f"D {kind} N={N} {setting}", setting, lay, *random_inputs(B, H, N, d, 5000 + N), d ** -0.5, GATES[BF],
                guards=True)


# ---- E. dense shapes on the variable-length kernels (ops.attn_fwd / attn_bwd) -------------------------------------------
def run_ops(monkeypatch, qkv, do, B, N, H, d, scale):
    """ops.attn_fwd + ops.attn_bwd with every buffer they allocate pre-filled with NaN; returns o, lse, dqkv, delta."""
    made = []

    def nan_empty(shape, dtype, like):
        t = torch.full(shape, float("nan"), dtype=dtype, device=like.device)
        made.append(t)
        return t

    with monkeypatch.context() as m:
        m.setattr(ops, "empty", nan_empty)
        o, lse = ops.attn_fwd(qkv, B, N, H, d, scale)
        n0 = len(made)
        dqkv = ops.attn_bwd(qkv, o, do, lse, B, N, H, d, scale)
    assert tuple(lse.shape) == (H, B * N), "expected the variable-length kernels (lse (H, B*N))"
    delta = [t for t in made[n0:] if t.dtype == F32 and tuple(t.shape) == (H, B * N)]
    assert len(delta) == 1
    return o, lse, dqkv, delta[0]


def ops_views(qkv, do, o, lse, dqkv, delta, B, N, H, d):
    split = lambda t, i, n: t.view(B, N, n, H, d)[:, :, i].permute(0, 2, 1, 3)
    ins = {"q": split(qkv, 0, 3), "k": split(qkv, 1, 3), "v": split(qkv, 2, 3), "do": split(do, 0, 1)}
    outs = {"o": split(o, 0, 1), "dq": split(dqkv, 0, 3), "dk": split(dqkv, 1, 3), "dv": split(dqkv, 2, 3),
            "lse": lse.view(H, B, N).permute(1, 0, 2), "delta": delta.view(H, B, N).permute(1, 0, 2)}
    return ins, outs


CELLS_E = [(d, N) for d in (32, 48, 80, 96) for N in (1, 16, 17, 63, 64, 65, 128, 129, 481, 577)] + [(64, N) for N in (481, 577, 1025)]


@pytest.mark.parametrize("d,N", CELLS_E)
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
def test_dense_shapes_on_varlen_kernels(d, N, dtype, monkeypatch):
    use(monkeypatch, "default")
    B, H = 3, 2
    I = H * d
    scale = d ** -0.5
    g = gen(6000 + 7 * d + N)
    qkv = randn((B * N, 3 * I), g, 1.5).to(dtype)
    do = randn((B * N, I), g).to(dtype)
    o, lse, dqkv, delta = run_ops(monkeypatch, qkv, do, B, N, H, d, scale)
    ins, outs = ops_views(qkv, do, o, lse, dqkv, delta, B, N, H, d)
    judge(f"E d={d} N={N} {dtype}", ins, outs, scale, GATES[dtype])
    o2, lse2, dqkv2, delta2 = run_ops(monkeypatch, qkv, do, B, N, H, d, scale)
    assert torch.equal(bits(o), bits(o2)) and torch.equal(bits(lse), bits(lse2)) and torch.equal(bits(dqkv), bits(dqkv2))


def test_config5_extents_on_varlen_kernels(monkeypatch):
    """BASELINE config 5's attention (ViT-H/14 at 224^2: B = 256, H = 16, N = 577, dim_head 80; 147,712 tokens, 1.1 GB of qkv):
    the 64-bit offset arithmetic of attention_varlen.hip at the size the ViT-H bench rows run.  Every item against float64 in
    chunks of 8 images, the whole tensor too, bit-identical run to run."""
    use(monkeypatch, "default")
    B, H, N, d = 256, 16, 577, 80
    I = H * d
    scale = d ** -0.5
    g = gen(7000)
    qkv = randn((B * N, 3 * I), g, 1.5).to(BF)
    do = randn((B * N, I), g).to(BF)
    o, lse, dqkv, delta = run_ops(monkeypatch, qkv, do, B, N, H, d, scale)
    ins, outs = ops_views(qkv, do, o, lse, dqkv, delta, B, N, H, d)
    judge("E config5", ins, outs, scale, GATES[BF], chunk=8)
    o2, lse2, dqkv2, _ = run_ops(monkeypatch, qkv, do, B, N, H, d, scale)
    assert torch.equal(bits(o), bits(o2)) and torch.equal(bits(lse), bits(lse2)) and torch.equal(bits(dqkv), bits(dqkv2))
