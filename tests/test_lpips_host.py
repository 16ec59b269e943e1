"""Host-side tests of the LPIPS head's C ABI and of the LPIPS / loss modules on their torch route (no GPU needed).

Fixtures: tests/golden/g30_lpips_head.npz, g31_lpips_loss.npz, g31_lpips_keys.json (tests/golden/make_golden_lpips.py)."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import lpips_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("lpips_head_workspace_bytes", "lpips_head_f32", "lpips_head_backward_f32")


def _lib():
    from pit_hip import _lib as L

    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


@pytest.fixture(scope="module")
def g30():
    return np.load(os.path.join(G, "g30_lpips_head.npz"))


@pytest.fixture(scope="module")
def g31():
    return np.load(os.path.join(G, "g31_lpips_loss.npz"))


def test_symbols_are_exported_bound_and_declared():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "gqhip.h")).read()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and name in L._SIGNATURES and hasattr(dll, name) and hasattr(L.lib(), name)
        assert re.search(r"^(?:int|int64_t)\s+%s\s*\(" % name, header, flags=re.M), name
    assert L.lib().gqhip_abi_version() == L.ABI_VERSION == 8
    assert "#define GQHIP_ABI_VERSION 8" in header


def test_workspace_size_function():
    lib = _lib().lib()
    assert lib.lpips_head_workspace_bytes(0, 64, 16) == 0
    assert lib.lpips_head_workspace_bytes(16, 64, 65536) > 0 and lib.lpips_head_workspace_bytes(16, 64, 65536) % 256 == 0
    for bad in ((1, 0, 4), (1, 513, 4), (1, 64, 0), (-1, 64, 4), (1 << 15, 64, 1 << 15)):
        assert lib.lpips_head_workspace_bytes(*bad) == -1, bad
    # a tile never owns fewer partial sums than images it can touch: HW = 1, 64-pixel tiles, 64 images each
    assert lib.lpips_head_workspace_bytes(1000, 8, 1) >= 1000 * 8


def test_statuses_without_a_device():
    """Expected statuses, written here, for made-up pointers that are never dereferenced because nothing can launch without a device
    (then a call that gets past its checks returns 3).  SAFETY: never where a HIP device is present -- it skips there."""
    if torch.cuda.is_available():
        pytest.skip("passes made-up pointers: safe only where no kernel can launch")
    lib = _lib().lib()
    fake, ample = 0x10000, 1 << 40
    B, C, HW = 2, 64, 323
    need = lib.lpips_head_workspace_bytes(B, C, HW)
    assert need > 0

    def fwd(f0=fake, f1=fake, w=fake, keep=None, out=fake, B=B, C=C, HW=HW, layout=0, ws=fake, ws_bytes=ample):
        return lib.lpips_head_f32(f0, f1, w, keep, 2.0, out, B, C, HW, layout, ws, ws_bytes, None)

    def bwd(f0=fake, f1=fake, w=fake, keep=None, g=fake, grad=fake, B=B, C=C, HW=HW, layout=0):
        return lib.lpips_head_backward_f32(f0, f1, w, keep, 2.0, g, grad, B, C, HW, layout, None)

    for fn, ptrs in ((fwd, ("f0", "f1", "w", "out")), (bwd, ("f0", "f1", "w", "g", "grad"))):
        for p in ptrs:
            assert fn(**{p: None}) == 1, (fn.__name__, p)
        for bad in (dict(C=0), dict(C=513), dict(HW=0), dict(B=-1), dict(layout=2), dict(layout=-1), dict(B=1 << 15, HW=1 << 15)):
            assert fn(**bad) == 1, (fn.__name__, bad)
        assert fn(f0=fake + 2) == 1                       # 4-byte alignment is required
        for layout in (0, 1):
            assert fn(layout=layout) == 3                  # would launch
            assert fn(layout=layout, f0=fake + 4) == 3     # 16-byte alignment only picks the wider kernel
            assert fn(layout=layout, keep=fake + 1) == 3
        assert fn(C=1) == 3 and fn(C=512) == 3 and fn(HW=1) == 3
    assert fwd(B=0, ws=None, ws_bytes=0) == 0 and bwd(B=0) == 0
    assert fwd(B=0, f0=None) == 1                          # the order of the checks: arguments before "nothing to do"
    assert fwd(ws=None) == 2 and fwd(ws_bytes=need - 1) == 2 and fwd(ws=fake + 8) == 2
    assert fwd(ws_bytes=need) == 3


def test_restatement_reproduces_the_reference_in_fp64(g30):
    """lpips_ref.head_ref against the reference's own ops in fp64 (g30), to 1e-3 unit: the GPU tests may lean on it.  Where the
    reference's gradient is NaN (a pixel whose f1 is all zero) the restatement holds the limit."""
    worst_o = worst_g = 0.0
    for shape, near, masked in R.CASES:
        cid = R.case_id(shape, near, masked).replace("/", ".")
        f0, f1, w, keep, g = R.case_inputs(shape, near, masked)
        out, grad, uo, ug = R.head_ref(f0, f1, w, keep, R.KEEP_SCALE, g)
        sel = R.grad_sample(grad.numel())
        want = torch.from_numpy(g30[cid + ".grad_f64"])
        got, unit = grad.reshape(-1)[sel], ug.reshape(-1)[sel]
        fin = torch.isfinite(want)
        assert torch.isfinite(grad).all()
        zero_pixels = (torch.from_numpy(f1).double().pow(2).sum(1, keepdim=True) == 0).expand(*shape).reshape(-1)[sel]
        assert bool((zero_pixels | fin).all()), cid       # the reference is NaN only where f1's pixel is all zero
        eo = R.err_units(out, g30[cid + ".out_f64"], uo)
        eg = R.err_units(got[fin], want[fin], unit[fin])
        worst_o, worst_g = max(worst_o, eo), max(worst_g, eg)
        assert eo <= 1e-3 and eg <= 1e-3, (cid, eo, eg)
    print(f"restatement vs reference fp64: out {worst_o:.2e} unit, grad {worst_g:.2e} unit")


def test_torch_route_against_the_reference(g31):
    """LPIPS and GeneralLPIPSWithDiscriminator on the torch route (CPU) against the reference's own run: every output within
    2 x the reference's fp32-vs-fp64 error (floor: one fp32 rounding of its largest magnitude); bit-equality is printed."""
    R.run_loss_against_fixture(g31, torch.device("cpu"))


def test_state_dict_keys_and_shapes_equal_the_reference():
    from pit_hip.modules.lpips.loss.lpips import LPIPS

    want = json.load(open(os.path.join(G, "g31_lpips_keys.json")))
    assert [[k, list(v.shape)] for k, v in LPIPS().state_dict().items()] == want["lpips"]
    assert [[k, list(v.shape)] for k, v in R.loss_module().state_dict().items()] == want["loss"]
    assert all(not p.requires_grad for p in LPIPS().parameters())
    from pit_hip.modules.lpips.model.model import NLayerDiscriminator

    keys = list(NLayerDiscriminator(use_actnorm=True).state_dict())
    assert "main.3.loc" in keys and "main.3.scale" in keys and "main.2.bias" in keys


def _tiny_engine(**extra):
    from pit_hip.util import instantiate_from_config, load_config

    cfg = copy.deepcopy(load_config(os.path.join(G, "tiny_config.yaml"))["model"])
    cfg["params"].update(extra)
    cfg["params"]["loss_config"]["params"]["disc_start"] = 0
    return instantiate_from_config(cfg)


def _fill_loss(engine):
    engine.loss.perceptual_loss.load_state_dict(R.fill_state(engine.loss.perceptual_loss.state_dict(), R.SEED_LPIPS))
    engine.loss.discriminator.load_state_dict(R.fill_state(engine.loss.discriminator.state_dict(), R.SEED_DISC))


def test_default_construction_has_no_loss():
    m = _tiny_engine()
    assert not hasattr(m, "loss") and not any(k.startswith("loss.") for k in m.state_dict())
    with pytest.raises(RuntimeError, match="eval_only=False"):
        m.get_discriminator_params()


def test_checkpoint_restores_the_loss(tmp_path):
    src = _tiny_engine(eval_only=False)
    _fill_loss(src)
    path = str(tmp_path / "engine.ckpt")
    torch.save({"state_dict": src.state_dict()}, path)
    dst = _tiny_engine(eval_only=False)
    assert not dst.loss.perceptual_loss.weights_loaded
    missing, unexpected = dst.init_from_ckpt(path)
    assert not missing and not unexpected and dst.loss.perceptual_loss.weights_loaded
    want = src.state_dict()
    assert any(k.startswith("loss.perceptual_loss.net.") for k in want) and "loss.logvar" in want
    for k, v in dst.state_dict().items():
        assert torch.equal(v, want[k]), k
    # through the constructor too; a checkpoint without loss.* keys leaves the perceptual loss unusable
    assert _tiny_engine(eval_only=False, ckpt_path=path).loss.perceptual_loss.weights_loaded
    torch.save({"state_dict": {k: v for k, v in want.items() if not k.startswith("loss.")}}, path)
    assert not _tiny_engine(eval_only=False, ckpt_path=path).loss.perceptual_loss.weights_loaded


def test_weight_loading_failures(tmp_path):
    from pit_hip.modules.lpips.loss.lpips import LPIPS

    x = torch.zeros(1, 3, 16, 16)
    m = LPIPS()
    with pytest.raises(RuntimeError, match="no weights"):
        m(x, x)
    missing = str(tmp_path / "nowhere" / "vgg.pth")
    with pytest.raises(FileNotFoundError, match=re.escape(missing)):
        m.load_from_pretrained(missing)
    # local files: the lin weights alone do not make a perceptual loss, with a torchvision-style vgg16 state_dict they do
    full = R.fill_state(m.state_dict(), R.SEED_LPIPS)
    lin_path, vgg_path = str(tmp_path / "vgg.pth"), str(tmp_path / "vgg16.pth")
    torch.save({k: v for k, v in full.items() if k.startswith("lin")}, lin_path)
    torch.save({"features." + k.split(".", 2)[2]: v for k, v in full.items() if k.startswith("net.")}, vgg_path)
    m.load_from_pretrained(lin_path)
    with pytest.raises(RuntimeError, match=r"net\.\*"):
        m(x, x)
    with pytest.raises(FileNotFoundError):
        m.load_from_pretrained(lin_path, missing)
    m.load_from_pretrained(lin_path, vgg_path)
    assert m.weights_loaded and all(torch.equal(v, full[k]) for k, v in m.state_dict().items())
    assert LPIPS(pretrained=False)(x, x).shape == (1, 1, 1, 1)


def test_refusals():
    from pit_hip.modules.losses.discriminator_loss import GeneralLPIPSWithDiscriminator as Loss

    with pytest.raises(NotImplementedError):
        Loss(disc_start=0, dims=3)
    with pytest.raises(NotImplementedError):
        Loss(disc_start=0, scale_input_to_tgt_size=True)
    loss = R.loss_module()
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="VF"):
        loss(x, x, regularization_log={"zp": x, "aux_feature": x}, optimizer_idx=0, global_step=0, last_layer=None)
    with pytest.raises(NotImplementedError):
        loss.log_images(x, x)
    with pytest.raises(NotImplementedError):
        loss(x, x, regularization_log={}, optimizer_idx=2, global_step=0, last_layer=None)


def test_training_step_changes_the_right_group_only():
    torch.manual_seed(0)
    m = _tiny_engine(eval_only=False).train()
    _fill_loss(m)
    m.loss.perceptual_loss.eval()
    ae, disc = m.get_autoencoder_params(), m.get_discriminator_params()
    assert ae and disc and not {id(p) for p in ae} & {id(p) for p in disc}
    assert {id(p) for p in disc} == {id(p) for p in m.loss.discriminator.parameters()}
    opts = [torch.optim.Adam([p for p in ae if p.requires_grad], lr=1e-3), torch.optim.Adam(disc, lr=1e-3)]
    batch = {"img": torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1}
    frozen = [p.detach().clone() for p in m.loss.perceptual_loss.parameters()]
    for idx, (mine, other) in enumerate(((ae, disc), (disc, ae))):
        before_mine, before_other = [p.detach().clone() for p in mine], [p.detach().clone() for p in other]
        for o in opts:
            o.zero_grad(set_to_none=True)
        loss, log = m.inner_training_step(batch, 0, optimizer_idx=idx, global_step=1)
        assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in log.values())
        assert ("train/loss/total" in log) == (idx == 0) and ("train/loss/disc" in log) == (idx == 1)
        loss.backward()
        opts[idx].step()
        assert any(not torch.equal(a, b) for a, b in zip(before_mine, mine))
        assert all(torch.equal(a, b) for a, b in zip(before_other, other))
    assert all(torch.equal(a, b) for a, b in zip(frozen, m.loss.perceptual_loss.parameters()))
