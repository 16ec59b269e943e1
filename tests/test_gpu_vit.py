"""-m gpu: the BSQ-ViT backbone on a real MI355X -- the fused attention kernel (csrc/gq_attn.h, _lib.mha_fwd) against an fp64
restatement, its determinism, the g21 goldens through the modules, the full-size bsqvit_gq_0.25 encoder on both routes, and
which calls enter the kernel."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.convstack]
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
GATE = 4e-6      # max|O - O_fp64| <= GATE * max|v|, per head


def _qkv(B, H, L, seed, d=64):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(B, L, 3 * H * d, device=DEV, generator=g)


def _ref64(qkv, H):
    """fp64 softmax(q k^T / sqrt(d)) v per (batch, head) on the device (tests/attn_ref.py's formula), [B, L, E] fp64."""
    B, L, E3 = qkv.shape
    E = E3 // 3
    d = E // H
    out = torch.empty(B, L, E, dtype=torch.float64, device=qkv.device)
    for b in range(B):
        q, k, v = (qkv[b, :, i * E:(i + 1) * E].double().reshape(L, H, d).transpose(0, 1) for i in range(3))
        p = torch.softmax(q @ k.transpose(1, 2) / d ** 0.5, dim=-1)
        out[b] = (p @ v).transpose(0, 1).reshape(L, E)
    return out


def _sdpa32(qkv, H):
    B, L, E3 = qkv.shape
    E = E3 // 3
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, L, H, E // H).transpose(1, 2) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, E)


def _check(qkv, H, label):
    from pit_hip import _lib

    B, L, E3 = qkv.shape
    E = E3 // 3
    d = E // H
    out = _lib.mha_fwd(qkv, H)
    torch.cuda.synchronize()
    ref = _ref64(qkv, H)
    err = (out.double() - ref).abs().reshape(B, L, H, d).amax(dim=(0, 1, 3))
    terr = (_sdpa32(qkv, H).double() - ref).abs().reshape(B, L, H, d).amax(dim=(0, 1, 3))
    vmax = qkv[..., 2 * E:].abs().reshape(B, L, H, d).amax(dim=(0, 1, 3)).double()
    rel, trel = float((err / vmax).max()), float((terr / vmax).max())
    print(f"{label}: max|O - O64| / max|v| = {rel:.3e} (torch fp32 SDPA {trel:.3e})")
    assert bool(torch.isfinite(out).all())
    assert rel <= GATE, label
    return out


@pytest.mark.parametrize("B,H,L", [(16, 12, 1024), (2, 12, 4096), (2, 3, 1), (2, 3, 63), (2, 3, 65), (2, 3, 81), (2, 3, 1000),
                                   (1, 1, 333)])
def test_mha_kernel_against_fp64(B, H, L):
    _check(_qkv(B, H, L, seed=B * 1000 + H * 10 + L), H, f"B{B} H{H} L{L}")


def _heads(qkv, H):
    """views of q, k, v as [B, L, H, d]"""
    B, L, E3 = qkv.shape
    E = E3 // 3
    return [qkv[..., i * E:(i + 1) * E].view(B, L, H, E // H) for i in range(3)]


@pytest.mark.parametrize("f", [-12, 8])
def test_mha_kernel_operand_scaling(f):
    """q x 2^f, k x 2^-f, v x 2^f: the logits are unchanged, the operands span 2^+-f -- the gate is relative to max|v|."""
    qkv = _qkv(2, 12, 1024, seed=7)
    q, k, v = _heads(qkv, 12)
    q.mul_(2.0 ** f)
    k.mul_(2.0 ** -f)
    v.mul_(2.0 ** f)
    _check(qkv, 12, f"operands x 2^{f}")


def test_mha_kernel_whole_input_scaled_down():
    """The base case x 2^-12 (logits x 2^-24: a flat softmax, the output is the mean of v)."""
    _check(_qkv(2, 12, 1024, seed=8) * 2.0 ** -12, 12, "qkv x 2^-12")


def test_mha_kernel_peaked_softmax():
    """Every query is 7 x one key: its logit is ~ +56 .. +90 (7 |k|^2 / 8), the others ~ N(0, 7^2); no near ties."""
    B, H, L = 2, 4, 1024
    qkv = _qkv(B, H, L, seed=9)
    q, k, v = _heads(qkv, H)
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(1)).to(DEV)
    q.copy_(7.0 * k[:, perm])
    s = (q[0, :, 0] @ k[0, :, 0].T) / 8
    print(f"peaked: logits in [{float(s.min()):.1f}, {float(s.max()):.1f}]")
    assert float(s.max()) > 50
    _check(qkv, H, "peaked")


def test_mha_kernel_zero_q_is_mean_of_v():
    qkv = _qkv(2, 3, 81, seed=10)
    q, k, v = _heads(qkv, 3)
    q.zero_()
    out = _check(qkv, 3, "q = 0")
    assert torch.allclose(out.view(2, 81, 3, 64), v.mean(dim=1, keepdim=True).expand(-1, 81, -1, -1), rtol=0, atol=1e-6)


def test_mha_kernel_one_loud_head():
    """Head 5 is 2^10 times the others (v x 2^10, q x 2^5, k x 2^-5): the per-head gate holds on every head."""
    qkv = _qkv(2, 12, 1024, seed=11)
    q, k, v = _heads(qkv, 12)
    v[:, :, 5].mul_(2.0 ** 10)
    q[:, :, 5].mul_(2.0 ** 5)
    k[:, :, 5].mul_(2.0 ** -5)
    _check(qkv, 12, "one head x 2^10")


def test_mha_kernel_rejects_unbuilt_head_dims():
    from pit_hip import _lib

    with pytest.raises(_lib.GqHipError):
        _lib.mha_fwd(torch.zeros(1, 8, 3 * 96, device=DEV), 3)      # d = 32
    with pytest.raises(_lib.GqHipError):
        _lib.mha_fwd(torch.zeros(1, 8, 3 * 128, device=DEV), 3)     # E not divisible by heads
    with pytest.raises(_lib.GqHipError):
        _lib.mha_fwd(torch.zeros(8, 3 * 128, device=DEV), 2)        # not [B, L, 3E]


def test_mha_kernel_deterministic():
    from pit_hip import _lib

    qkv = _qkv(4, 12, 1024, seed=12)
    a = _lib.mha_fwd(qkv, 12)
    b = _lib.mha_fwd(qkv, 12)
    assert torch.equal(a, b)


# ---- modules ----------------------------------------------------------------------------------------------------------------
def _load_case(tag):
    from pit_hip.modules.vit import TransformerDecoder, TransformerEncoder

    d = np.load(os.path.join(G, f"g21_vit_{tag}.npz"))
    params = json.loads(str(d["params"]))
    enc, dec = TransformerEncoder(**params["enc"]).eval(), TransformerDecoder(**params["dec"]).eval()
    for pre, m in (("enc.", enc), ("dec.", dec)):
        m.load_state_dict({k[len(pre):]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith(pre)})
    return d, enc.to(DEV), dec.to(DEV)


class _Count:
    def __init__(self, monkeypatch):
        from pit_hip import _lib

        self.n, real = 0, _lib.mha_fwd

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)

        monkeypatch.setattr(_lib, "mha_fwd", counted)


@pytest.mark.parametrize("tag", ["d64_tail", "block_causal", "group4"])
def test_g21_goldens_on_the_gpu(tag, monkeypatch):
    from pit_hip.quantization.gaussian import GaussianQuantRegularizer

    cnt = _Count(monkeypatch)
    d, enc, dec = _load_case(tag)
    group = 4 if tag == "group4" else 16
    with torch.no_grad():
        z = enc(torch.from_numpy(d["x"]).to(DEV))
        reg = GaussianQuantRegularizer("blc", int(d["n_samples"]), group=group, backend="hip").eval().to(DEV)
        zhat, info = reg(z)
        rec = dec(torch.from_numpy(d["zhat"]).to(DEV))
    torch.cuda.synchronize()
    # the masked case stays on torch's route; the unmasked ones use the kernel (one call per layer and module)
    assert cnt.n == (0 if tag == "block_causal" else 2), cnt.n
    dz = float((z.cpu() - torch.from_numpy(d["z"])).abs().max())
    drec = float((rec.cpu() - torch.from_numpy(d["rec"])).abs().max())
    ind = info["indices"].cpu().numpy().reshape(-1)
    diff = ind != d["indices"].reshape(-1)
    print(f"{tag}: max|dz| {dz:.2e}  max|drec| {drec:.2e}  indices differing {int(diff.sum())} / {ind.size}")
    assert dz <= 5e-5 and drec <= 1e-4
    assert int(diff.sum()) <= 2 * max(1, ind.size // 1024) and np.all(d["gap"][diff] < 1e-3)


def test_graph_capture_replays_the_eager_encoder_bit_for_bit():
    d, enc, _ = _load_case("d64_tail")
    x = torch.from_numpy(d["x"]).to(DEV)
    with torch.no_grad():
        eager = enc(x)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            enc(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = enc(x)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def _bsqvit(name="0.25"):
    from pit_hip.util import instantiate_from_config, load_config

    cfg = load_config(os.path.join(G, f"bsqvit_gq_{name}.yaml"))
    torch.manual_seed(0)
    return instantiate_from_config(cfg["model"]).eval().to(DEV)


def test_full_size_vit_b_hip_route_against_torch_route(monkeypatch):
    from pit_hip.modules import vit

    eng = _bsqvit()
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(5)).to(DEV) * 2 - 1
    with torch.no_grad():
        z_hip = eng.encoder(x)
        # per-layer growth of the difference between the routes, on the same layer inputs
        enc = eng.encoder
        h = enc.ln_pre(enc.conv1(vit._patchify(x, 8, 8)) + enc.positional_embedding)
        growth = []
        for r in enc.transformer.resblocks:
            a = r.forward_hip(h)
            b = r(h.permute(1, 0, 2)).permute(1, 0, 2)
            growth.append(float((a - b).abs().max() / b.abs().max()))
            h = b
        monkeypatch.setattr(vit, "HIP_ATTN", False)
        z_torch = eng.encoder(x)
    rel = float((z_hip - z_torch).abs().max() / z_torch.abs().max())
    print(f"bsqvit_gq_0.25 bs 2 256^2: max|dz| / max|z| = {rel:.3e}; per-layer (one block, same input): "
          + " ".join(f"{g:.1e}" for g in growth))
    assert z_hip.shape == (2, 1024, 32)
    assert rel <= 1e-4


def test_routes_autograd_masks_and_flag_never_enter_the_kernel(monkeypatch):
    from pit_hip.modules import vit

    cnt = _Count(monkeypatch)
    d, enc, dec = _load_case("d64_tail")
    x = torch.from_numpy(d["x"]).to(DEV)
    z = enc(x)                                   # autograd: torch's MHA
    z.sum().backward()
    assert cnt.n == 0
    _, menc, _ = _load_case("block_causal")
    with torch.no_grad():
        menc(x)                                   # masked
        monkeypatch.setattr(vit, "HIP_ATTN", False)
        z_t = enc(x)                              # flag off
        assert cnt.n == 0
        monkeypatch.setattr(vit, "HIP_ATTN", True)
        z_h = enc(x)
        enc.cpu()(x.cpu())                        # CPU
    assert cnt.n == 1
    assert float((z_h - z_t).abs().max()) <= 5e-5
