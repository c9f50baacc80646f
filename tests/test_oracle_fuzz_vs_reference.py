"""CPU: the oracle against the REFERENCE ITSELF on the seeded random configurations the GPU fuzz tests use (tests/test_fuzz_gpu.py).
The committed goldens pin the oracle on fixed cases; the fuzz leans on it for rectangular patches, 1 / 4 channels, mean pooling, free
dim_head, ragged NaViT packs -- so those exact draws were executed through the unmodified reference modules and a fixed sample of their
outputs stored in tests/golden/fuzz_draws.npz (oracle/make_golden.py::main_fuzz: up to 1024 output entries and 64 entries of every
gradient tensor, smaller ones whole).  On those entries: logits within 1e-5 and every gradient within 1e-4 relative L2 in float32, and
the error of the oracle's pure-bf16 run (the yardstick of the fuzz's 1.5x gate) of the same size as the error of the reference's own
bf16 run (factor 3 either way: at these model sizes a few hundred roundings decide either figure; the BASELINE-width goldens carry the
reference's own bf16 numbers instead)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_fuzz_gpu as F  # noqa: E402  (the draws; importing it needs no GPU)
from oracle import navit_oracle as NO  # noqa: E402
from oracle import vit_oracle as O  # noqa: E402
from oracle.params import make_images, make_navit_images, make_navit_params, make_params, sample_index  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "fuzz_draws.npz"))
DRAWS = json.loads(bytes(GOLD["draws"]).decode())
SAMPLE, LOGITS_SAMPLE = 64, 1024        # oracle/make_golden.py::FUZZ_SAMPLE / FUZZ_LOGITS_SAMPLE


def rel(a, b):
    a = a.detach().double().flatten(); b = b.detach().double().flatten()
    n = b.norm().item()
    return (a - b).norm().item() / (n if n > 0 else 1.0)


def _sampled(t, n):
    return t.detach().flatten()[torch.from_numpy(sample_index(t.numel(), n))]


def _check_grads(tag, grads, what):
    """The golden's gradient samples are concatenated in the reference's parameter order (DRAWS[tag]["grads"]: name, numel)."""
    layout = DRAWS[tag]["grads"]
    assert sorted(k for k, _ in layout) == sorted(grads), (what, layout, sorted(grads))
    ref_all, at = torch.from_numpy(GOLD[f"{tag}::gsample"]), 0
    for k, numel in layout:
        assert grads[k].numel() == numel, (k, *what)
        ref = ref_all[at:at + min(numel, SAMPLE)]
        at += ref.numel()
        if numel:
            assert rel(_sampled(grads[k], SAMPLE), ref) <= 1e-4, (k, *what, rel(_sampled(grads[k], SAMPLE), ref))
    assert at == ref_all.numel()


@pytest.mark.parametrize("seed", range(F.N_DRAWS))
def test_oracle_equals_reference_on_fuzz_draw(seed):
    kind, cfg, batch = F.draw(seed)
    assert json.loads(json.dumps([kind, cfg, batch])) == DRAWS[str(seed)]["draw"], "the draw changed: regenerate tests/golden/fuzz_draws.npz"
    params = make_params(kind, cfg, 50 + seed)
    img = make_images(cfg, batch, 1050 + seed)
    out, grads = O.run_fwd_bwd(kind, cfg, params, img, torch.float32)
    ref_out = torch.from_numpy(GOLD[f"{seed}::logits"])
    assert list(out.shape) == DRAWS[str(seed)]["logits_shape"]
    assert rel(_sampled(out, LOGITS_SAMPLE), ref_out) <= 1e-5, (kind, cfg, batch)
    _check_grads(str(seed), grads, (kind, cfg, batch))
    if seed % 4 == 0:       # the bf16 yardstick on a quarter of the draws
        o16, g16 = O.run_fwd_bwd(kind, cfg, params, img, torch.bfloat16)
        r16 = torch.from_numpy(GOLD[f"{seed}::bf16::logits"])
        e_o, e_r = rel(_sampled(o16, LOGITS_SAMPLE), ref_out), rel(r16, ref_out)
        assert e_o <= 3 * e_r + 1e-3 and e_r <= 3 * e_o + 1e-3, (e_o, e_r)      # same size (small models: a few hundred roundings decide either figure)


@pytest.mark.parametrize("seed", range(8))
def test_navit_oracle_equals_reference_on_fuzz_draw(seed):
    cfg, packs = F.draw_navit(seed)
    assert json.loads(json.dumps([cfg, packs])) == DRAWS[f"navit{seed}"]["draw"], "the draw changed: regenerate tests/golden/fuzz_draws.npz"
    params = make_navit_params(cfg, 90 + seed)
    images = make_navit_images(cfg, packs, 1090 + seed)
    out, grads = NO.run_fwd_bwd(cfg, params, images, torch.float32)
    ref = torch.from_numpy(GOLD[f"navit{seed}::logits"])
    assert list(out.shape) == DRAWS[f"navit{seed}"]["logits_shape"]
    assert rel(_sampled(out, LOGITS_SAMPLE), ref) <= 1e-5, (cfg, packs)
    _check_grads(f"navit{seed}", grads, (cfg, packs))
