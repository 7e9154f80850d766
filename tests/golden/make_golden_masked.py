"""Fixtures of the occlusion-masked decoder (mask_flow = mask_corr = True) from the REFERENCE's
own modules: ``make_golden``'s ``gen_e2e`` / ``gen_train`` with only the two decoder flags
overridden (everything else — the shims, the stand-ins, the inputs and seeds — is make_golden's).

    python tests/golden/make_golden_masked.py

writes
* ``golden_e2e_masked_b2_s256_it4.npz`` (+ ``..._flow_pred.npz``): the keys of
  ``golden_e2e_b2_s256_it4.npz``; ``flow_pred_last`` — 1 MiB of incompressible floats on its
  own — is kept in a file of its own so that no fixture exceeds the repository's 1 MiB limit;
* ``golden_train_masked_b2_s256_it3.npz``: the keys of ``golden_train_b2_s256_it2.npz``,
  detach_mask=True, 3 iterations (with 2 the predicted mask is used once and never crosses a
  second detach).

The generator refuses to write a fixture whose low-resolution masks are saturated (at most half
of the values inside (0.05, 0.95)): such a fixture would not exercise the masking.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

E2E = "golden_e2e_masked_b2_s256_it4"
TRAIN = "golden_train_masked_b2_s256_it3"
TRAIN_LABELS = (4, 9)  # the plain training fixture's: no symmetric class, no stand-in involved


def masked_decoder_cfg(ref, iters=4, feat_size=None, _plain=mg.decoder_cfg):
    cfg = _plain(ref, iters, feat_size)
    assert cfg["detach_mask"] is True
    cfg.update(mask_flow=True, mask_corr=True)
    return cfg


class MaskWatch:
    """Records every single-channel sigmoid output — the decoder's low-resolution masks
    (scflow_decoder.py:213-214) — while active."""

    def __enter__(self):
        self.seen = []
        self._sigmoid = torch.sigmoid

        def sigmoid(x, *a, **kw):
            y = self._sigmoid(x, *a, **kw)
            if y.dim() == 4 and y.shape[1] == 1:
                self.seen.append(y.detach())
            return y
        torch.sigmoid = sigmoid
        return self

    def __exit__(self, *exc):
        torch.sigmoid = self._sigmoid

    def check(self, iters):
        assert len(self.seen) == iters, f"{len(self.seen)} masks seen, {iters} iterations"
        for i, m in enumerate(self.seen[:-1]):  # the last one masks nothing
            frac = float(((m > 0.05) & (m < 0.95)).float().mean())
            print(f"  mask {i}: min {float(m.min()):.3f} max {float(m.max()):.3f}, "
                  f"{100 * frac:.1f} % in (0.05, 0.95)")
            assert frac > 0.5, f"iteration {i}: saturated mask ({frac:.3f} inside (0.05, 0.95))"


def save(name, out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}.npz: {size} bytes")
    assert size <= 1 << 20, f"{name}.npz is larger than 1 MiB"


def main():
    ref = mg.load_reference()
    mg.decoder_cfg = masked_decoder_cfg
    torch.manual_seed(0)
    e2e = {}
    with MaskWatch() as w:
        mg.gen_e2e(ref, e2e, B=2, S=256, iters=4)
    w.check(4)
    save(E2E + "_flow_pred", {"flow_pred_last": e2e.pop("flow_pred_last")})
    save(E2E, e2e)
    tr = {}
    with MaskWatch() as w:
        mg.gen_train(ref, tr, TRAIN_LABELS, B=2, S=256, iters=3)
    w.check(3)
    save(TRAIN, tr)


if __name__ == "__main__":
    main()
