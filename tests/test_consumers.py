"""Consumers of the encoder's internals: the reference's Recorder (recorder.py:26-29), Extractor
(extractor.py:50-57), Dino's NetWrapper (dino.py:134-151) and T2TViT (t2t.py:45, 57) wired around the drop-in modules.

CPU part: the hook points those wrappers look up, restated -- every `Attention.attend` under `transformer` (found by isinstance), the
`transformer` attribute, `children()[-2]` = `to_latent`, and `Transformer` built with t2t.py's arguments -- must exist on the drop-in
and take / release forward hooks.  GPU part: the same wiring run end to end against the un-hooked fused path."""
import pytest
import torch


def _tiny_vit():
    from vit_pytorch_amd import ViT
    return ViT(image_size=32, patch_size=8, num_classes=5, dim=32, depth=3, heads=2, dim_head=16, mlp_dim=64)


def test_reference_recorder_finds_every_attend_module():
    """recorder.py:7-8, 26-31: every module of `vit.transformer` that is an `Attention` gets a forward hook on its `attend`; eject
    (recorder.py:33-38) removes them and hands back the model."""
    from vit_pytorch_amd.vit import Attention
    v = _tiny_vit()
    hooks = [m.attend.register_forward_hook(lambda *_: None) for m in v.transformer.modules() if isinstance(m, Attention)]
    assert len(hooks) == 3
    attends = [m.attend for m in v.transformer.modules() if isinstance(m, Attention)]
    assert len(attends) == 3 and all(len(a._forward_hooks) == 1 for a in attends)
    for h in hooks:
        h.remove()
    assert all(len(a._forward_hooks) == 0 for a in attends)


def test_reference_extractor_and_netwrapper_find_their_layers():
    """extractor.py:50-59: a forward hook on the `transformer` attribute; dino.py:134-140 with layer = -2: `children()[-2]`."""
    v = _tiny_vit()
    assert hasattr(v, "transformer")
    h = v.transformer.register_forward_hook(lambda *_: None)
    assert len(v.transformer._forward_hooks) == 1
    h.remove()
    assert len(v.transformer._forward_hooks) == 0
    assert [*v.children()][-2] is v.to_latent
    from vit_pytorch_amd import SimpleViT
    s = SimpleViT(image_size=32, patch_size=8, num_classes=5, dim=32, depth=1, heads=2, dim_head=16, mlp_dim=64)
    assert [*s.children()][-2] is s.to_latent


def test_reference_t2t_vit_builds_on_the_drop_in_transformer():
    """t2t.py:5 imports vit_pytorch.vit.Transformer.  T2TViT(image_size=64, dim=64, depth=2, heads=2, mlp_dim=128) with its default
    t2t_layers ((7, 4), (3, 2), (3, 2)) and 3 channels builds two token-to-token layers by keyword (t2t.py:45: dim = heads' width =
    mlp_dim = 3 * 7 * 7 = 147 and 147 * 3 * 3 = 1323, heads = 1, depth = 1; the third t2t layer is an Identity) and its main
    transformer POSITIONALLY (t2t.py:57: Transformer(dim, depth, heads, dim_head, mlp_dim, dropout)) -- the drop-in must accept both."""
    import vit_pytorch_amd.vit as mine
    channels, ts = 3, []
    for i, (kernel, _stride) in enumerate(((7, 4), (3, 2), (3, 2))):
        channels *= kernel ** 2
        if i < 2:
            ts.append(mine.Transformer(dim=channels, heads=1, depth=1, dim_head=channels, mlp_dim=channels, dropout=0.))
    ts.append(mine.Transformer(64, 2, 2, 64, 128, 0.))
    assert all(isinstance(t, mine.Transformer) for t in ts)
    assert sorted(t.norm.weight.shape[0] for t in ts) == [64, 147, 1323]
    assert len(ts[2].layers) == 2
    for t in ts[:2]:
        assert isinstance(t.layers[0][0].to_out, torch.nn.Identity)      # heads == 1 and dim_head == dim (vit.py:45)


# ---- GPU: the same wiring, end to end ------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _rel(a, b):
    a = a.detach().double().flatten().cpu(); b = b.detach().double().flatten().cpu()
    return ((a - b).norm() / b.norm()).item()


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_recorder_wiring_end_to_end(dtype):
    from vit_pytorch_amd.vit import Attention
    torch.manual_seed(0)
    v = _tiny_vit().to("cuda", dtype=dtype).eval()
    img = torch.randn(2, 3, 32, 32, device="cuda").to(dtype)
    plain = v(img)
    recordings = []
    hooks = [m.attend.register_forward_hook(lambda _m, _i, o: recordings.append(o.clone().detach()))
             for m in v.transformer.modules() if isinstance(m, Attention)]
    pred = v(img)
    attns = torch.stack(recordings, dim=1)                # recorder.py:57-59
    for h in hooks:
        h.remove()
    assert tuple(attns.shape) == (2, 3, 2, 17, 17)        # (batch, depth, heads, n, n)
    assert torch.allclose(attns.float().sum(-1), torch.ones(2, 3, 2, 17, device="cuda"), atol=2e-2 if dtype == torch.bfloat16 else 1e-5)
    assert _rel(pred, plain) < (3e-2 if dtype == torch.bfloat16 else 1e-5)


@gpu
def test_extractor_and_netwrapper_wiring_end_to_end():
    torch.manual_seed(0)
    v = _tiny_vit().to("cuda").eval()
    img = torch.randn(2, 3, 32, 32, device="cuda")
    plain = v(img)
    got = {}
    h1 = v.transformer.register_forward_hook(lambda _m, _i, o: got.__setitem__("latents", o.clone().detach()))     # extractor.py:46-48
    h2 = [*v.children()][-2].register_forward_hook(lambda _m, i, o: got.__setitem__("hidden", o.flatten(1)))       # dino.py:142-144
    pred = v(img)
    h1.remove(); h2.remove()
    assert tuple(got["latents"].shape) == (2, 17, 32) and tuple(got["hidden"].shape) == (2, 32)
    assert _rel(got["hidden"], got["latents"][:, 0]) < 1e-6        # pool = cls: to_latent sees the cls row of the transformer output
    assert _rel(pred, plain) < 1e-5
    assert _rel(v.mlp_head(got["hidden"]), plain) < 1e-5


def _torch_block(t, x, r, dim, heads, dim_head):
    """The block of `t` in plain torch (vit.py:51-64, 18-25, 78-83), float64: output and input gradient for the cotangent r."""
    B, N = x.shape[:2]
    attn, ff = t.layers[0]
    xd = x.detach().double().requires_grad_(True)
    ln = lambda z, m: torch.nn.functional.layer_norm(z, (dim,), m.weight.double(), m.bias.double())
    h = ln(xd, attn.norm)
    q, k, vv = (h @ attn.to_qkv.weight.double().t()).chunk(3, dim=-1)
    sp = lambda z: z.view(B, N, heads, dim_head).transpose(1, 2)
    a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * dim_head ** -0.5, dim=-1) @ sp(vv)
    a = a.transpose(1, 2).reshape(B, N, heads * dim_head)
    if not isinstance(attn.to_out, torch.nn.Identity):
        a = a @ attn.to_out[0].weight.double().t() + attn.to_out[0].bias.double()
    x1 = a + xd
    f = ff.net
    h2 = torch.nn.functional.gelu(ln(x1, f[0]) @ f[1].weight.double().t() + f[1].bias.double())
    x2 = h2 @ f[4].weight.double().t() + f[4].bias.double() + x1
    ref = ln(x2, t.norm)
    (ref * r.double()).sum().backward()
    return ref, xd.grad


@gpu
def test_standalone_transformer_as_t2t_and_mae_use_it():
    """t2t.py:45 builds Transformer(dim = d, heads = 1, depth = 1, dim_head = d, mlp_dim = d) with d = 3 * 7 * 7 = 147 and
    147 * 9 = 1323: one head as wide as the model, an Identity output projection, and widths that are NOT multiples of 4 (they
    run op by op on the any-width kernels); mae.py:37 builds an ordinary decoder Transformer."""
    from vit_pytorch_amd.vit import Transformer
    torch.manual_seed(0)
    for dim, heads, dim_head in ((147, 1, 147), (1323, 1, 1323), (144, 1, 144), (64, 4, 16)):
        t = Transformer(dim=dim, depth=1, heads=heads, dim_head=dim_head, mlp_dim=dim).to("cuda")
        x = torch.randn(2, 49, dim, device="cuda", requires_grad=True)
        r = torch.randn(2, 49, dim, device="cuda")      # a generic cotangent (mean(y^2) of a LayerNorm output with gamma = 1, beta = 0
        y = t(x)                                        # has an analytically ZERO input gradient: pure cancellation, not a test)
        (y * r).sum().backward()
        ref, gref = _torch_block(t, x, r, dim, heads, dim_head)
        assert _rel(y, ref) < 1e-5 and _rel(x.grad, gref) < 1e-4, (dim, _rel(y, ref), _rel(x.grad, gref))
        for p_ in t.parameters():
            assert p_.grad is not None and torch.isfinite(p_.grad).all()


@gpu
def test_t2t_width_in_bfloat16():
    """The same odd-width block with 16-bit parameters: every op of the op-by-op path has an element-at-a-time form."""
    from vit_pytorch_amd.vit import Transformer
    torch.manual_seed(1)
    dim = 147
    t32 = Transformer(dim=dim, depth=1, heads=1, dim_head=dim, mlp_dim=dim).to("cuda")
    t = Transformer(dim=dim, depth=1, heads=1, dim_head=dim, mlp_dim=dim).to("cuda")
    t.load_state_dict(t32.state_dict())
    t = t.to(torch.bfloat16)
    x = torch.randn(2, 81, dim, device="cuda")
    r = torch.randn(2, 81, dim, device="cuda")
    xb = x.to(torch.bfloat16).requires_grad_(True)
    y = t(xb)
    (y.float() * r).sum().backward()
    ref, gref = _torch_block(t32, x, r, dim, 1, dim)
    assert _rel(y, ref) < 3e-2 and _rel(xb.grad, gref) < 6e-2, (_rel(y, ref), _rel(xb.grad, gref))
