"""FID goldens (same rules as make_golden*.py: build container only, imports /root/reference, stores DATA).

  g32_fid.npz   five feature fixtures, each a pair of fp32 blocks x, y = x + noise of shape [n, D] at (D, n) = (8, 64), (48, 400),
                (64, 500), (100, 300), (256, 2000): relu'd, correlated Gaussians with mean about 0.3.  Per fixture k:
                  f{k}.x, f{k}.y            the features
                  f{k}.mu_x, f{k}.cov_x     np.mean(x, axis=0) (fp32, as numpy returns it for an fp32 block) and np.cov(x, rowvar=False)
                                            (fp64), as eval.py:248 forms them
                  f{k}.mu_y, f{k}.cov_y     the same of y
                  f{k}.fid                  the reference's calculate_frechet_distance(mu_y, cov_y, mu_x, cov_x)
                The last fixture's x and y are in g32_fid_f4_{x,y}{0,1}.npz (key "rows": its first and second 1000 rows) and its two
                covariances in g32_fid_f4_cov.npz as their upper triangles, row by row (np.cov's result is symmetric bit for bit):
                no committed file is larger than 1 MiB.  tests/fid_ref.py:load_fixtures reassembles all five.
                Every fixture has n > D; the generator asserts that the reference stays on its main path on them (no eps retry, no
                complex part)."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from pit.evaluations.fid.fid_score import calculate_frechet_distance  # noqa: E402
from scipy import linalg  # noqa: E402

SHAPES = ((8, 64), (48, 400), (64, 500), (100, 300), (256, 2000))   # (D, n)
SEED = 3200


def features(D, n, rng):
    mix = rng.standard_normal((D, D)) / np.sqrt(D)
    scale = 0.2 + 0.6 * rng.random(D)
    x = np.maximum(rng.standard_normal((n, D)) @ mix * scale + 0.3, 0.0).astype(np.float32)
    noise = (0.05 * scale * rng.standard_normal((n, D))).astype(np.float32)
    return x, np.maximum(x + noise, 0.0).astype(np.float32)


def main():
    out = {}
    for k, (D, n) in enumerate(SHAPES):
        x, y = features(D, n, np.random.default_rng(SEED + k))
        mu_x, cov_x = np.mean(x, axis=0), np.cov(x, rowvar=False)      # eval.py:248,257 on the fp32 blocks: an fp32 mean, an fp64 cov
        mu_y, cov_y = np.mean(y, axis=0), np.cov(y, rowvar=False)
        assert mu_x.dtype == np.float32 and cov_x.dtype == np.float64
        covmean, _ = linalg.sqrtm(cov_y.dot(cov_x), disp=False)
        assert np.isfinite(covmean).all() and not np.iscomplexobj(covmean), (D, n)      # the reference's main path
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            fid = calculate_frechet_distance(mu_y, cov_y, mu_x, cov_x)
        assert said.getvalue() == "", said.getvalue()
        out.update({f"f{k}.x": x, f"f{k}.y": y, f"f{k}.mu_x": mu_x, f"f{k}.cov_x": cov_x, f"f{k}.mu_y": mu_y, f"f{k}.cov_y": cov_y,
                    f"f{k}.fid": np.float64(fid)})
        print(f"f{k}: D={D} n={n} mean {x.mean():.3f} fid {fid:.6f}")
    # no committed file above 1 MiB: the largest fixture's feature blocks go to files of their own, in halves, and its two
    # covariances (symmetric bit for bit) as their upper triangles; tests/fid_ref.py:load_fixtures puts them together again
    big = len(SHAPES) - 1
    paths = []
    for name in ("x", "y"):
        rows = out.pop(f"f{big}.{name}")
        half = rows.shape[0] // 2
        for h, part in enumerate((rows[:half], rows[half:])):
            paths.append(os.path.join(HERE, f"g32_fid_f{big}_{name}{h}.npz"))
            np.savez_compressed(paths[-1], rows=part)
    tri = {}
    for name in ("cov_x", "cov_y"):
        c = out.pop(f"f{big}.{name}")
        assert np.array_equal(c, c.T)
        tri[name] = c[np.triu_indices(c.shape[0])]
    paths.append(os.path.join(HERE, f"g32_fid_f{big}_cov.npz"))
    np.savez_compressed(paths[-1], **tri)
    paths.append(os.path.join(HERE, "g32_fid.npz"))
    np.savez_compressed(paths[-1], **out)
    for p in paths:
        print(os.path.basename(p), os.path.getsize(p))
        assert os.path.getsize(p) < 1 << 20, p


if __name__ == "__main__":
    main()
