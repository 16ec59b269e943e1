"""CPU: the BSQ-ViT backbone port (pit_hip.modules.vit) against the reference's goldens (tests/golden/g21_vit_*.npz, written by
make_golden_vit.py), the shipped bsqvit YAMLs through the config factory, and the fp64 attention restatement."""
import json
import os

import numpy as np
import pytest
import torch

import attn_ref

G = os.path.join(os.path.dirname(__file__), "golden")
CASES = ("d64_tail", "block_causal", "group4")


def load_case(tag):
    from pit_hip.modules.vit import TransformerDecoder, TransformerEncoder

    d = np.load(os.path.join(G, f"g21_vit_{tag}.npz"))
    params = json.loads(str(d["params"]))
    enc, dec = TransformerEncoder(**params["enc"]).eval(), TransformerDecoder(**params["dec"]).eval()
    for pre, m in (("enc.", enc), ("dec.", dec)):
        sd = {k[len(pre):]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith(pre)}
        assert list(sd) == list(m.state_dict()), "state_dict keys / order differ from the reference's"
        m.load_state_dict(sd, strict=True)
    return d, enc, dec


@pytest.mark.parametrize("tag", CASES)
def test_g21_encoder_and_decoder_bit_identical_to_reference(tag):
    """The torch route (CPU) is the reference's op sequence: z and the reconstruction from the reference's zhat, bit for bit."""
    d, enc, dec = load_case(tag)
    with torch.no_grad():
        z = enc(torch.from_numpy(d["x"]))
        rec = dec(torch.from_numpy(d["zhat"]))
    assert z.shape == d["z"].shape and np.array_equal(z.numpy(), d["z"])
    assert rec.shape == d["rec"].shape and np.array_equal(rec.numpy(), d["rec"])


def test_g21_block_causal_mask_is_not_all_enabled():
    from pit_hip.modules.vit import get_attention_mask

    d, enc, _ = load_case("block_causal")
    assert enc.mask_type == "block-causal" and enc.mask_block_size == 9
    m = get_attention_mask(81, "cpu", mask_type="block-causal", block_size=9)
    assert m.dtype == torch.bool and m.shape == (81, 81) and 0 < int(m.sum()) < 81 * 81
    assert get_attention_mask(81, "cpu", mask_type="none") is None
    # the mask changes the result: the same weights without it give another z
    enc.mask_type = "none"
    with torch.no_grad():
        assert not torch.equal(enc(torch.from_numpy(d["x"])), torch.from_numpy(d["z"]))


def test_g21_autograd_matches_no_grad():
    """Autograd takes the same torch route: same values as under no_grad, and gradients reach in_proj_weight."""
    d, enc, _ = load_case("d64_tail")
    x = torch.from_numpy(d["x"])
    z = enc(x)
    assert np.array_equal(z.detach().numpy(), d["z"])
    z.square().sum().backward()
    g = enc.transformer.resblocks[0].attn.in_proj_weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_cpu_and_autograd_never_enter_the_kernel(monkeypatch):
    from pit_hip import _lib
    from pit_hip.modules import vit

    def boom(*a, **k):
        raise AssertionError("the HIP kernel was entered")

    monkeypatch.setattr(_lib, "mha_fwd", boom)
    assert vit.HIP_ATTN is True
    d, enc, dec = load_case("group4")
    with torch.no_grad():
        assert np.array_equal(enc(torch.from_numpy(d["x"])).numpy(), d["z"])
    enc(torch.from_numpy(d["x"]))


def _engine(name):
    from pit_hip.util import instantiate_from_config, load_config

    cfg = load_config(os.path.join(G, f"bsqvit_gq_{name}.yaml"))
    return cfg, instantiate_from_config(cfg["model"])


@pytest.mark.parametrize("name,group", [("0.25", 16), ("0.50", 8), ("1.00", 4)])
def test_bsqvit_yaml_instantiates_with_the_reference_state_dict_layout(name, group):
    from pit_hip.models.autoencoder import AutoencodingEngine
    from pit_hip.modules.vit import TransformerDecoder, TransformerEncoder

    cfg, eng = _engine(name)
    assert isinstance(eng, AutoencodingEngine)
    assert isinstance(eng.encoder, TransformerEncoder) and isinstance(eng.decoder, TransformerDecoder)
    assert eng.regularization.format == "blc" and eng.regularization.group == group
    keys = json.load(open(os.path.join(G, "g21_vit_keys.json")))
    for part in ("encoder", "decoder"):
        got = [[k, list(v.shape)] for k, v in getattr(eng, part).state_dict().items()]
        assert got == keys[part], part


def test_bsqvit_0_25_shapes_at_256():
    _, eng = _engine("0.25")
    eng.eval()
    torch.manual_seed(0)
    with torch.no_grad():
        z = eng.encoder(torch.rand(1, 3, 256, 256) * 2 - 1)
        assert z.shape == (1, 1024, 32)
        rec = eng.decoder(torch.randn(1, 1024, 16))
    assert rec.shape == (1, 3, 256, 256) and bool(torch.isfinite(rec).all())


def test_timm_replacements():
    from pit_hip.modules import vit

    assert vit.to_2tuple(8) == (8, 8) and vit.to_2tuple([4, 2]) == (4, 2)
    torch.manual_seed(3)
    a = vit.trunc_normal_(torch.empty(4096), std=0.02)
    torch.manual_seed(3)
    b = torch.nn.init.trunc_normal_(torch.empty(4096), std=0.02)
    assert torch.equal(a, b) and float(a.abs().max()) <= 2.0
    dp = vit.DropPath(0.5).eval()
    x = torch.randn(4, 3)
    assert dp(x) is x
    dp.train()
    y = dp(x)
    assert all(torch.equal(r, 0 * r) or torch.allclose(r, 2 * x[i]) for i, r in enumerate(y))


@pytest.mark.parametrize("L,heads", [(1, 1), (17, 2), (81, 2), (64, 3)])
def test_attn_ref_matches_torch_mha_fp64(L, heads):
    E = 64 * heads
    torch.manual_seed(L + heads)
    mha = torch.nn.MultiheadAttention(E, heads).double().eval()
    with torch.no_grad():
        mha.in_proj_bias.normal_(0, 0.1)
        mha.out_proj.bias.normal_(0, 0.1)
    x = torch.randn(3, L, E, dtype=torch.float64)
    with torch.no_grad():
        want = mha(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), need_weights=False)[0].transpose(0, 1)
    got = attn_ref.mha(x.numpy(), mha.in_proj_weight.detach().numpy(), mha.in_proj_bias.detach().numpy(),
                       mha.out_proj.weight.detach().numpy(), mha.out_proj.bias.detach().numpy(), heads)
    assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))


def test_mha_fwd_rejects_bad_shapes_without_a_device():
    from pit_hip import _lib

    with pytest.raises(_lib.GqHipError):
        _lib.mha_fwd(torch.zeros(1, 4, 3 * 128), 2)          # CPU tensor: no fallback
