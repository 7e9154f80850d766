"""CPU: the RAFT baseline's training path.

* the pure-torch restatement (tests/raft_train_restatement.py) in float64 reproduces the fixture
  written from the reference's own modules (tests/golden/make_golden_raft_train.py);
* the gather-form adjoint of the convex upsampling (what scflow_convex_upsample_bwd implements)
  equals torch autograd;
* ``raft_refiner_train_forward`` (scflow_amd/train/model.py) reproduces the fixture with
  tests/test_train_host.py's torch stand-ins for the HIP ops plus one for the convex upsampling —
  the wiring (detach, heads, loss weights, sequence weighting), at the GPU test's tolerances;
* the C ABI declares the new entry consistently, the ABI version is unchanged, and the loss
  configurations the path does not restate are refused before any device work.
"""
import re

import numpy as np
import pytest
import torch

from tests import raft_restatement as rr
from tests import raft_train_restatement as rt
from tests.test_abi import HEADER
from tests.test_train_host import _patch_torch_ops, train_batch

orc = pytest.importorskip("oracle.scflow_oracle")

TAGS = ("mask", "plain", "bilinear")


def _batch(dtype):
    B, S, _, seed, labels, _ = rt.fixture_meta()
    batch, _, _ = train_batch(B, S, seed=seed, labels=labels, dtype=dtype)
    return batch


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_reference_fixture(tag):
    g = rt.raft_train_golden()
    _, _, iters, _, _, lc = rt.fixture_meta()
    sd = {k: v.requires_grad_(True) for k, v in rt.train_state_dict(tag, torch.float64).items()}
    kind, _, _, over = rt.VARIANTS[tag]
    res = rt.raft_train_forward(sd, _batch(torch.float64), iters,
                                occlusion=kind == "RAFTRefinerFlowMask",
                                convex=over.get("convex_unsample_flow", True), **lc)
    res["loss"].backward()
    got = [res["loss"].item(), res["loss_flow"].item()] + \
        ([] if res["loss_occ"] is None else [res["loss_occ"].item()])
    np.testing.assert_allclose(got, g[f"{tag}_losses"], rtol=1e-6)
    np.testing.assert_allclose([v.item() for v in res["seq_flow"]], g[f"{tag}_seq_flow"], rtol=1e-6)
    np.testing.assert_allclose([v.item() for v in res["seq_occ"]], g[f"{tag}_seq_occ"], rtol=1e-6)
    gf = res["gt_flow"]
    stats = [gf.sum().item(), (gf >= lc["max_flow"]).sum().item(),
             gf[gf < lc["max_flow"]].abs().sum().item()]
    np.testing.assert_allclose(stats, g[f"{tag}_gt_flow_stats"], rtol=1e-6)
    for i, f in enumerate(res["lr_flow"]):
        assert rr.mean_epe(torch.from_numpy(g[f"{tag}_lr_flow"][i]), f.detach().float()) <= 1e-4
    ref = dict(zip([str(n) for n in g[f"{tag}_grad_names"]], g[f"{tag}_grad_norms"]))
    checked = 0
    for name, rv in ref.items():
        part, tail = name.split(".", 1)
        if part == "encoder":  # shared: the oracle holds it under both names
            grads = [sd["real_encoder." + tail].grad, sd["render_encoder." + tail].grad]
            grad = None if all(x is None for x in grads) else sum(x for x in grads if x is not None)
        else:
            grad = sd[name if part == "context" else tail].grad
        if np.isnan(rv):
            assert grad is None or float(grad.abs().max()) == 0.0, name
            continue
        assert grad is not None, name
        np.testing.assert_allclose(float(grad.norm()), rv, rtol=1e-6, atol=1e-9, err_msg=name)
        checked += 1
    assert checked == sum(not np.isnan(v) for v in ref.values()) and checked >= 120
    for b in rt.BIAS_GRADS:  # elementwise: what catches a wrong channel order
        if f"{tag}_grad_{b}" in g:
            want = g[f"{tag}_grad_{b}"]
            np.testing.assert_allclose(sd[b].grad.numpy(), want, rtol=1e-6,
                                       atol=1e-9 * (1 + float(np.abs(want).max())), err_msg=b)


@pytest.mark.parametrize("geom", [(1, 1, 1), (2, 3, 11), (1, 9, 8)], ids=lambda g: "n%d-%dx%d" % g)
@pytest.mark.parametrize("with_occ", [True, False])
def test_gather_form_adjoint_equals_autograd(geom, with_occ):
    n, h, w = geom
    g = torch.Generator().manual_seed(7 * h + w)
    f64 = torch.float64
    x = ((torch.rand(n, 2, h, w, generator=g, dtype=f64) - 0.5) * 6).requires_grad_()
    logits = (torch.randn(n, 576, h, w, generator=g, dtype=f64) * 8).requires_grad_()
    occ = torch.rand(n, 1, h, w, generator=g, dtype=f64).requires_grad_() if with_occ else None
    g_flow = torch.randn(n, 2, 8 * h, 8 * w, generator=g, dtype=f64)
    g_occ = torch.randn(n, 1, 8 * h, 8 * w, generator=g, dtype=f64) if with_occ else None
    obj = (rr.convex_upsample(x, logits, 0.25, 8.0) * g_flow).sum()
    if with_occ:
        obj = obj + (rr.convex_upsample(occ, logits, 0.25, 1.0) * g_occ).sum()
    obj.backward()
    with torch.no_grad():
        dx, dlogits, docc = rt.convex_upsample_adjoint(x, logits, occ, g_flow, g_occ, 0.25, 8.0)
    torch.testing.assert_close(dx, x.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(dlogits, logits.grad, rtol=0, atol=1e-12)
    if with_occ:
        torch.testing.assert_close(docc, occ.grad, rtol=0, atol=1e-12)
    else:
        assert docc is None


def _patch_convex(monkeypatch):
    from scflow_amd.train import model

    def convex(x, logits, occ=None, logit_scale=.25, value_scale=8.):
        nchw = lambda a: a.permute(0, 3, 1, 2)  # noqa: E731
        up = rr.convex_upsample(nchw(x), nchw(logits), logit_scale, value_scale)
        upo = None if occ is None else rr.convex_upsample(nchw(occ), nchw(logits), logit_scale, 1.0)
        return up, upo
    monkeypatch.setattr(model, "convex_upsample", convex)


@pytest.mark.parametrize("tag", TAGS)
def test_train_forward_host_matches_reference_fixture(monkeypatch, tag):
    from scflow_amd.train.model import raft_refiner_train_forward
    _patch_torch_ops(monkeypatch)
    _patch_convex(monkeypatch)
    r = rt.build_train_refiner(tag, dtype=torch.float64)
    res = raft_refiner_train_forward(r, _batch(torch.float64))
    res["loss"].backward()
    assert set(res) == {"loss", "loss_flow", "loss_occ", "seq_flow_losses", "seq_occ_losses", "outs",
                        "gt_flow"}
    rt.check_against_fixture(tag, res, r)
    assert int(r.context.norm1.num_batches_tracked) == 1  # BN in train mode


def test_c_abi_declares_the_backward_consistently(monkeypatch):
    from scflow_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+scflow_convex_upsample_bwd\s*\(([^)]*)\)\s*;", src)
    assert m, "include/scflow_hip.h does not declare scflow_convex_upsample_bwd"
    n_args = len(m.group(1).split(","))
    restype, argtypes = _lib.SIGNATURES["scflow_convex_upsample_bwd"]
    assert len(argtypes) == n_args and restype is _lib.c_int
    sent = {}
    monkeypatch.setattr(ops, "_require", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_launch", lambda name, dev, *args: sent.update(name=name, n=len(args)))
    n, h, w = 1, 2, 3
    dlg, dx, docc = ops.convex_upsample_backward(
        ops.Chan.whole(torch.zeros(n * h * w, 576)), torch.zeros(n * h * w, 2),
        torch.zeros(n * h * w, 1), torch.zeros(n, 2, 8 * h, 8 * w), None, n, h, w)
    assert sent == dict(name="scflow_convex_upsample_bwd", n=n_args - 1)  # + the stream
    assert dlg.shape == (6, 576) and dx.shape == (6, 2) and docc.shape == (6, 1)


def test_abi_version_is_still_4():
    from scflow_amd import _lib
    src = open(HEADER).read()
    assert re.search(r"#define\s+SCFLOW_ABI_VERSION\s+4\b", src)
    assert _lib.load().scflow_abi_version() == 4


def _with_cfg(tag, **over):
    from scflow_amd import MODELS
    return MODELS.build(rt.model_cfg(tag, 1, **over))


@pytest.mark.parametrize("tag,over", [
    ("mask", dict(flow_loss_cfg=None)),
    ("mask", dict(occlusion_loss_cfg=None)),
    ("plain", dict(loss_cfg=None)),
    ("mask", dict(filter_invalid_flow_by_depth=True)),
    ("mask", dict(flow_loss_cfg=dict(type="MultiLevelEPE", gamma=0.8,
                                     loss_func_cfg=dict(type="RAFTLoss")))),
    ("mask", dict(flow_loss_cfg=dict(type="SequenceLoss", gamma=0.8,
                                     loss_func_cfg=dict(type="L1Loss", loss_weight=1.0)))),
    ("mask", dict(occlusion_loss_cfg=dict(type="SequenceLoss", gamma=0.8,
                                          loss_func_cfg=dict(type="RAFTLoss", loss_weight=1.0)))),
    ("plain", dict(loss_cfg=dict(type="SequenceLoss", gamma=0.8,
                                 loss_func_cfg=dict(type="DisentanglePointMatchingLoss")))),
], ids=lambda v: v if isinstance(v, str) else "-".join(v))
def test_unsupported_loss_configs_are_refused_before_device_work(tag, over):
    """No HIP op is patched here: reaching one on the CPU would raise ScflowError, not this."""
    from scflow_amd.train.model import raft_refiner_train_forward
    from scflow_amd.train.step import TrainStep
    r = _with_cfg(tag, **over)
    batch = {k: torch.zeros(1) for k in ("render_images", "real_images")}
    with pytest.raises(NotImplementedError):
        raft_refiner_train_forward(r, batch)
    with pytest.raises(NotImplementedError):
        r.loss(batch)
    with pytest.raises(NotImplementedError):
        TrainStep(r, None, None)


def test_loss_needs_a_gpu_and_graph_mode_is_refused():
    from scflow_amd._lib import ScflowError
    from scflow_amd.train.step import TrainStep
    r = _with_cfg("mask")
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ScflowError):
        r.loss(dict(render_images=x, real_images=x))
    with pytest.raises(NotImplementedError, match="graph"):
        TrainStep(r, None, None, graph=True)
