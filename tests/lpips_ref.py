"""What the LPIPS head and loss tests share: an fp64 torch restatement of csrc/lpips_head.h's formulas, the case table, the error
unit and deterministic generators (np.random.default_rng(seed)) for features, weights and images.

Unit of error: 2^-24 x sum |terms| of the quantity in question --
    out[b]:       (1 / HW) sum_p sum_c |w_c| m_c s u_c^2
    grad_f1_j:    (|g| / HW) (r1 |t_j| + |f1_j| r1^2 / n1 sum_c |t_c f1_c|)
so "1 unit" is one fp32 rounding of the sum of the magnitudes that were added."""
from __future__ import annotations

import numpy as np
import torch

U24 = 2.0 ** -24
# (B, C, H, W): the smallest shapes that can still go wrong -- odd HW, HW below a tile (several images per tile), C below, at and
# off the 16-byte chunk, one pixel, three images
SHAPES = [(2, 64, 17, 19), (2, 128, 9, 9), (3, 256, 2, 2), (2, 512, 5, 7), (1, 512, 1, 1), (2, 3, 4, 5), (2, 192, 3, 3)]
MULTI_BLOCK_SHAPE = (2, 64, 40, 40)     # several tiles contribute to one image; held against the restatement only
KEEP_SCALE = 2.0
SEED_LPIPS, SEED_DISC, SEED_IMAGES = 31, 32, 33      # of g31 (tests/golden/make_golden_lpips.py)


def case_id(shape, near, masked):
    return "x".join(map(str, shape)) + ("/near" if near else "/indep") + ("/keep" if masked else "/all")


CASES = [(s, near, masked) for s in SHAPES for near in (False, True) for masked in (False, True)]


def features(rng, shape):
    """post-ReLU-like: non-negative, about half zeros, fp32"""
    return np.maximum(rng.standard_normal(shape), 0.0).astype(np.float32)


def case_inputs(shape, near, masked):
    """f0, f1 [B, C, H, W] fp32, w [C] fp32 of mixed signs, keep uint8 or None, g [B] fp32 -- a function of the case alone"""
    B, C, H, W = shape
    rng = np.random.default_rng([B, C, H, W, int(near), int(masked)])
    f0 = features(rng, shape)
    if near:        # the operating point: a good reconstruction, where the difference of the two unit vectors cancels
        f1 = np.maximum(f0 + np.float32(0.05) * rng.standard_normal(shape).astype(np.float32), 0.0).astype(np.float32)
    else:
        f1 = features(rng, shape)
    w = rng.standard_normal(C).astype(np.float32)
    keep = (rng.random(shape) < 0.5).astype(np.uint8) if masked else None
    g = rng.standard_normal(B).astype(np.float32)
    return f0, f1, w, keep, g


def head_ref(f0, f1, w, keep=None, keep_scale=1.0, g=None):
    """The restatement in fp64: (out [B], grad_f1 [B, C, H, W], unit_out [B], unit_grad [B, C, H, W]); grad and its unit are None
    without ``g``.  Inputs: numpy or torch, logical [B, C, H, W]."""
    f0, f1 = (torch.as_tensor(np.asarray(t)).double() for t in (f0, f1))
    w = torch.as_tensor(np.asarray(w)).double().reshape(1, -1, 1, 1)
    ms = torch.ones_like(f0) if keep is None else torch.as_tensor(np.asarray(keep)).double() * float(keep_scale)
    HW = f0.shape[2] * f0.shape[3]
    n0, n1 = f0.pow(2).sum(1, keepdim=True).sqrt(), f1.pow(2).sum(1, keepdim=True).sqrt()
    r0, r1 = 1.0 / (n0 + 1e-10), 1.0 / (n1 + 1e-10)
    u = f0 * r0 - f1 * r1
    out = (w * ms * u * u).sum((1, 2, 3)) / HW
    unit_out = U24 * (w.abs() * ms * u * u).sum((1, 2, 3)) / HW
    if g is None:
        return out, None, unit_out, None
    gs = torch.as_tensor(np.asarray(g)).double().reshape(-1, 1, 1, 1) / HW
    t = -2.0 * w * ms * u
    dot = (t * f1).sum(1, keepdim=True)
    k = torch.where(n1 > 0, r1 * r1 / torch.where(n1 > 0, n1, torch.ones_like(n1)), torch.zeros_like(n1))
    grad = gs * (r1 * t - f1 * dot * k)
    unit_grad = U24 * gs.abs() * (r1 * t.abs() + f1.abs() * k * (t * f1).abs().sum(1, keepdim=True))
    return out, grad, unit_out, unit_grad


def err_units(got, want, unit):
    """max |got - want| / unit over the elements (0 / 0 = 0: an exact zero is no error)"""
    d = (torch.as_tensor(np.asarray(got)).double() - torch.as_tensor(np.asarray(want)).double()).abs().reshape(-1)
    unit = torch.as_tensor(np.asarray(unit)).double().reshape(-1)
    q = torch.where(d == 0, torch.zeros_like(d), d / unit)
    return float(q.max()) if q.numel() else 0.0


def grad_sample(n, most=2048):
    """the elements of a flattened gradient the fixture stores (a fixed stride; every element below ``most``)"""
    return np.arange(0, n, max(1, -(-n // most)))


def fill_state(state, seed, skip=("scaling_layer.",)):
    """A state_dict like ``state`` (name -> tensor; only shapes and names are read) with He-scaled convolution weights, small
    biases, BatchNorm weights near 1 and neutral running statistics, from ``seed`` alone."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in state.items():
        shape = tuple(v.shape)
        if any(k.startswith(s) for s in skip):
            out[k] = v.clone()
        elif k.endswith("num_batches_tracked") or k.endswith("initialized"):
            out[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            out[k] = torch.ones(shape)
        elif k.endswith("running_mean"):
            out[k] = torch.zeros(shape)
        elif len(shape) == 4 and shape[2:] == (1, 1) and shape[0] == 1:      # a `lin` layer: weights of either sign, O(1 / C)
            out[k] = torch.from_numpy((rng.standard_normal(shape) / shape[1]).astype(np.float32) + np.float32(1.0 / shape[1]))
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            out[k] = torch.from_numpy((rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32))
        elif k.endswith("bias"):
            out[k] = torch.from_numpy((0.01 * rng.standard_normal(shape)).astype(np.float32))
        else:                                                                 # a norm layer's weight / scale
            out[k] = torch.from_numpy((1.0 + 0.02 * rng.standard_normal(shape)).astype(np.float32))
    return out


def images(seed, B=2, size=32, cin=4):
    """(inputs [B, 3, size, size] in [-1, 1], decoder input [B, cin, size, size], stand-in decoder weight [3, cin, 3, 3]) fp32: the
    reconstruction is a 3x3 convolution of the decoder input, close to the inputs"""
    rng = np.random.default_rng(seed)
    x = (rng.random((B, 3, size, size)) * 2 - 1).astype(np.float32)
    h = np.zeros((B, cin, size, size), np.float32)
    h[:, :3] = x
    h[:, 3:] = rng.standard_normal((B, cin - 3, size, size)).astype(np.float32)
    wd = (0.02 * rng.standard_normal((3, cin, 3, 3))).astype(np.float32)
    for c in range(3):
        wd[c, c, 1, 1] += 1.0
    return torch.from_numpy(x), torch.from_numpy(h), torch.from_numpy(wd)


# ---- the LPIPS and loss modules against g31, on any device (the host test's torch route, the GPU test's two routes) ----
def bound_check(name, got, f32, f64):
    got, f32, f64 = (np.asarray(t, dtype=np.float64) for t in (got, f32, f64))
    ref_err = np.abs(f32 - f64).max()
    floor = U24 * np.abs(f64).max()
    err = np.abs(got - f64).max()
    print(f"{name}: err {err:.3e}, reference fp32 err {ref_err:.3e}, floor {floor:.3e}, bit-equal to the fp32 run: "
          f"{np.array_equal(got.astype(np.float32), f32.astype(np.float32))}")
    assert err <= 2 * max(ref_err, floor), name


def loss_module(dtype=torch.float32):
    from pit_hip.modules.losses.discriminator_loss import GeneralLPIPSWithDiscriminator

    loss = GeneralLPIPSWithDiscriminator(disc_start=0)
    loss.perceptual_loss.load_state_dict(fill_state(loss.perceptual_loss.state_dict(), SEED_LPIPS))
    loss.discriminator.load_state_dict(fill_state(loss.discriminator.state_dict(), SEED_DISC))
    loss = loss.to(dtype).train()
    loss.perceptual_loss.eval()
    return loss


def run_loss_against_fixture(g31, device, check=bound_check):
    """LPIPS and the loss module on ``device`` against g31 (shared with the GPU test)"""
    x, h, wd = (t.to(device) for t in images(SEED_IMAGES))
    dec = torch.nn.Conv2d(h.shape[1], 3, 3, padding=1, bias=False).to(device)
    dec.weight.data.copy_(wd)
    nodes = {}
    lp = loss_module().perceptual_loss.to(device)
    hh = h.clone().requires_grad_()
    out = lp(x, dec(hh))
    nodes["lpips"] = out
    assert out.shape == (2, 1, 1, 1)
    gvec = torch.tensor([1.0, -0.5], device=device).reshape(-1, 1, 1, 1)
    check("lpips.out", out.detach().reshape(-1).cpu(), g31["lpips.out_f32"], g31["lpips.out_f64"])
    check("lpips.grad_h", torch.autograd.grad((out * gvec).sum(), hh)[0].cpu(), g31["lpips.grad_h_f32"], g31["lpips.grad_h_f64"])
    for opt in (0, 1):
        loss = loss_module().to(device)
        loss.perceptual_loss.register_forward_hook(lambda m, i, o, opt=opt: nodes.__setitem__(f"opt{opt}.p_loss", o))
        hh = h.clone().requires_grad_()
        val, log = loss(x, dec(hh), regularization_log={}, optimizer_idx=opt, global_step=1, last_layer=dec.weight, split="train")
        check(f"opt{opt}.loss", val.detach().cpu(), g31[f"opt{opt}.loss_f32"], g31[f"opt{opt}.loss_f64"])
        want_keys = {k[len(f"opt{opt}.log."):-len("_f32")] for k in g31.files if k.startswith(f"opt{opt}.log.") and k.endswith("_f32")}
        assert {k.replace("/", ".") for k in log} == want_keys
        for k, v in log.items():
            kk = f"opt{opt}.log.{k.replace('/', '.')}"
            check(kk, v.detach().cpu(), g31[kk + "_f32"], g31[kk + "_f64"])
        if opt == 0:
            check("opt0.grad_h", torch.autograd.grad(val, hh)[0].cpu(), g31["opt0.grad_h_f32"], g31["opt0.grad_h_f64"])
        else:
            check("opt1.grad_disc0", torch.autograd.grad(val, loss.discriminator.main[0].weight)[0].cpu(),
                  g31["opt1.grad_disc0_f32"], g31["opt1.grad_disc0_f64"])
    return nodes
