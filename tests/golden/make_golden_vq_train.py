"""VQ train-step fixture (same rules as make_golden*.py: build container only, imports /root/reference, stores DATA).

  g24_vq_train_step.npz   two consecutive train() steps of the reference's VQQuantizer on the CPU under autograd, for the cases of
                      tests/vq_train_ref.py:CASES, with a plain SGD update of the codebook between them
                      (W1 = W0 - lr * grad, two fp32 ops; lr per case so that a chosen code moves about halfway to its items:
                      the second step's indices then depend on the update).  The codebook is drawn trained-like
                      (codes ~ N(0, 1) * 0.5), not the constructor's +-1/n, and rounded to fp16 values so that it can be stored
                      as float16 (exact; the file must stay under 1 MiB and 16 384 x 4 + 4096 x 8 + ... random fp32 words alone
                      are half of that).  z keeps full fp32 mantissas, so e - z rounds like any fp32 difference, and the
                      codebook of step 1 holds full fp32 rows wherever the update moved one; the arg-min on general fp32
                      codebooks is the subject of g16 / g20, not of this fixture.
                      loss = sum(z_q * w) + g_loss * info["codebook_loss"]; backward().
                      Stored: {tag}_emb (the codebook before step 0, float16), {tag}_lr; per step z, w, g_loss; z_q, indices,
                      codebook_loss, grad_z, grad_emb (the reference's fp32 autograd); gz64 / gz_abs, ge64 / ge_abs (the fp64
                      formulas of tests/vq_train_ref.py and the sum of |terms|); gz_ref_err / ge_ref_err =
                      max |reference fp32 grad - grad64| / (2^-24 grad_abs): the reference's own fp32 error.
                      The codebook before step 1 is emb - float32(lr) * grad_emb of step 0 in fp32 (asserted here bit for bit).
The "blc" case goes through the reference's "bchw" door: its own "blc" rearrange pattern ("b l c -> b h h c") is rejected by einops
(vq.py:49, as make_golden_r6.py found), and [B, L, c] IS the "b h w c" tensor the reference computes on, so z is handed over as
the [B, c, h, h] view of the same values and z_q, indices and z.grad are brought back to [B, L, .]: identical arithmetic.
Asserted here, else the next seed is tried: (i) the reference's indices equal oracle.vq_argmin_rows (the fp64 arbiter) on every row;
(ii) every row's fp64 top-2 distance gap exceeds 1e-4 (the existing VQ parity rule) -- so a GPU test can compare every element and
leave nothing out.  Also: some second-step index differs from the one the OLD codebook would give (a stale cache would show).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pit.quantization.vq import VQQuantizer as RefVQ  # noqa: E402

import vq_train_ref as R  # noqa: E402
from oracle import gq_oracle as O  # noqa: E402


def arbiter(z, emb, cfg):
    """(indices [items] of the fp64 arbiter, smallest top-2 gap)."""
    zi, _ = R.to_items(z, cfg)
    idx, best, second = O.vq_argmin_rows(np.ascontiguousarray(zi, np.float32), emb, with_gap=True)
    return idx, float((second - best).min())


def run_case(tag, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    ref = RefVQ("bchw", cfg["n"], cfg["dim"], beta=cfg["beta"], codebook_num=cfg["K"], legacy=cfg["legacy"]).train()
    blc = cfg["format"] == "blc"
    h = int(round(cfg["shape"][1] ** 0.5)) if blc else 0
    door = (lambda t: t.reshape(t.shape[0], h, h, -1).permute(0, 3, 1, 2)) if blc else (lambda t: t)          # [B, L, .] -> [B, ., h, h]
    home = (lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], h * h, -1).contiguous()) if blc else (lambda t: t)
    ref.embedding.weight.data = (0.5 * torch.randn(cfg["n"], cfg["dim"], generator=g)).half().float()
    N = int(np.prod(cfg["shape"]))
    b_coef = cfg["beta"] if cfg["legacy"] else 1.0
    lr = float(np.float32(0.5 / (R.G_LOSS[0] * b_coef * 2.0 / N)))
    emb0 = ref.embedding.weight.detach().numpy().copy()
    assert np.array_equal(emb0.astype(np.float16).astype(np.float32), emb0)
    out = {f"{tag}_emb": emb0.astype(np.float16), f"{tag}_lr": np.float64(lr)}
    moved = False
    for it in range(R.STEPS):
        z = 0.5 * torch.randn(cfg["shape"], generator=g)
        w = torch.randn(cfg["shape"], generator=g)
        g_loss = R.G_LOSS[it]
        emb = ref.embedding.weight.detach().numpy().copy()
        want_idx, gap = arbiter(z.numpy(), emb, cfg)
        if gap <= R.MIN_GAP:
            return None
        zt = z.clone().requires_grad_(True)
        ref.embedding.weight.grad = None
        zq, info = ref(door(zt))
        zq = home(zq)
        ((zq * w).sum() + g_loss * info["codebook_loss"]).backward()
        idx = home(info["indices"]).numpy()
        if not np.array_equal(R.idx_to_items(idx, cfg), want_idx):
            return None
        s = R.step(z.numpy(), emb, idx, cfg, w.numpy(), g_loss)
        gz, ge = zt.grad.numpy(), ref.embedding.weight.grad.numpy().copy()
        gz_err, ge_err = R.err_units(gz, s["grad_z"], s["grad_z_abs"]), R.err_units(ge, s["grad_emb"], s["grad_emb_abs"])
        assert abs(float(info["codebook_loss"].detach()) - s["loss"]) <= 2e-5 * max(1.0, abs(s["loss"]))
        assert np.abs(zq.detach().numpy() - s["e"]).max() <= 4 * R.U * np.abs(s["e"]).max() + 1e-7
        if it == 1:
            stale, _ = arbiter(z.numpy(), emb0, cfg)
            moved = bool((stale != want_idx).any())
        counts = np.bincount(want_idx, minlength=cfg["n"])
        print(f"{tag} step {it}: items {want_idx.size} codes used {int((counts > 0).sum())} max per code {int(counts.max())} "
              f"gap {gap:.2e} gz_ref_err {gz_err:.2f} ge_ref_err {ge_err:.2f}")
        p = f"{tag}_{it}_"
        out[p + "z"], out[p + "w"], out[p + "g_loss"] = z.numpy(), w.numpy(), np.float64(g_loss)
        out[p + "zq"], out[p + "indices"] = zq.detach().numpy(), idx
        out[p + "codebook_loss"] = np.float64(float(info["codebook_loss"].detach()))
        out[p + "grad_z"], out[p + "grad_emb"] = gz, ge
        out[p + "gz64"], out[p + "gz_abs"] = s["grad_z"], s["grad_z_abs"].astype(np.float32)
        out[p + "ge64"], out[p + "ge_abs"] = s["grad_emb"], s["grad_emb_abs"].astype(np.float32)
        out[p + "gz_ref_err"], out[p + "ge_ref_err"] = np.float64(gz_err), np.float64(ge_err)
        if it == 0:                                   # plain SGD, spelled as the two fp32 ops a test can repeat in numpy
            ref.embedding.weight.data = ref.embedding.weight.data - torch.tensor(lr, dtype=torch.float32) * ref.embedding.weight.grad
            again = (emb - np.float32(lr) * ge).astype(np.float32)
            assert np.array_equal(again, ref.embedding.weight.detach().numpy())
    return out if moved else None


if __name__ == "__main__":
    out = {}
    for i, (tag, cfg) in enumerate(R.CASES.items()):
        for seed in range(2400 + 1000 * i, 2400 + 1000 * i + 1000):
            got = run_case(tag, cfg, seed)
            if got is not None:
                break
        assert got is not None, tag
        out.update(got)
        out[f"{tag}_seed"] = np.int64(seed)
        print(f"{tag}: seed {seed}")
    path = os.path.join(HERE, "g24_vq_train_step.npz")
    np.savez_compressed(path, **out)
    print("max ref_err", max(float(v) for k, v in out.items() if k.endswith("ref_err")), "bytes", os.path.getsize(path))
