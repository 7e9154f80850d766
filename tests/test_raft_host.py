"""CPU: the RAFT baseline decoders' drop-in surface (registry, constructor, state dict, C ABI
plumbing) and the pin of the tests' pure-torch restatement to the reference's own outputs."""
import os
import re

import numpy as np
import pytest
import torch

from tests import raft_restatement as rr
from tests.helpers import t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["RAFTDecoder", "RAFTDecoderMask"])
def test_builds_from_reference_style_config(kind):
    from scflow_amd import MODELS, raft_decoder
    cls = getattr(raft_decoder, kind)
    by_name = MODELS.build(dict(type=kind, **rr.raft_decoder_cfg(12)))
    by_class = MODELS.build(dict(type=cls, **rr.raft_decoder_cfg(12)))
    for dec in (by_name, by_class):
        assert type(dec) is cls
        assert (dec.iters, dec.h_channels, dec.cxt_channels, dec.num_levels, dec.radius) == \
            (12, 128, 128, 4, 4)
        assert dec.mask_channels == 576 and dec.convex_upsample_flow is True
        for name in ("corr_block", "corr_lookup", "encoder", "gru", "flow_pred", "mask_pred"):
            assert isinstance(getattr(dec, name), torch.nn.Module), name
        assert hasattr(dec, "occlusion_pred") == (kind == "RAFTDecoderMask")
    # the reference's defaults: corr_lookup_cfg carries a `type`, the misspelt keyword is kept
    dec = cls(net_type="Basic", num_levels=4, radius=4, iters=3, convex_unsample_flow=False)
    assert dec.convex_upsample_flow is False and dec.corr_lookup.align_corners is True


@pytest.mark.parametrize("kind,tag", [("RAFTDecoder", "plain"), ("RAFTDecoderMask", "mask")])
def test_state_dict_is_the_references(kind, tag):
    dec = rr.build_raft_decoder(kind)
    ours = [(k, tuple(v.shape)) for k, v in dec.state_dict().items()]
    assert ours == rr.reference_state_shapes(tag)
    # a reference state dict loads strictly
    fresh = rr.build_raft_decoder(kind, seed=5, gain=1.0)
    fresh.load_state_dict(rr.raft_state_dict(tag), strict=True)
    for k, v in rr.raft_state_dict(tag).items():
        assert torch.equal(fresh.state_dict()[k], v), k


def test_refiners_are_registered():
    from scflow_amd import MODELS
    from scflow_amd.raft_refiner import RAFTRefinerFlow, RAFTRefinerFlowMask
    assert MODELS.get("RAFTRefinerFlow") is RAFTRefinerFlow
    assert MODELS.get("RAFTRefinerFlowMask") is RAFTRefinerFlowMask


def test_small_net_type_is_refused():
    from scflow_amd import MODELS
    for kind in ("RAFTDecoder", "RAFTDecoderMask"):
        with pytest.raises(NotImplementedError):
            MODELS.build(dict(type=kind, **rr.raft_decoder_cfg(4, net_type="Small")))


def test_header_and_binding_declare_convex_upsample():
    from scflow_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scflow_hip.h")).read(),
                 flags=re.S)
    assert re.search(r"\bint\s+scflow_convex_upsample\s*\(", src)
    assert "#define SCFLOW_ABI_VERSION 4" in src  # a new export only
    res, args = _lib.SIGNATURES["scflow_convex_upsample"]
    decl = re.search(r"scflow_convex_upsample\s*\((.*?)\)", src, flags=re.S).group(1)
    assert res is _lib.c_int and len(args) == len(decl.split(","))


def test_convex_upsample_rejects_bad_arguments_without_a_gpu():
    """Argument errors are return codes and launch nothing (no device is touched)."""
    from scflow_amd import _lib
    lib = _lib.load()
    p = 4096  # any non-NULL, 16-byte aligned value: never dereferenced on these paths
    ok = dict(logits=p, ls=576, lr=p, delta=p, occ=p, flow_up=p, occ_up=p, next0=p, s0=2, next1=p,
              s1=384, n=1, h=4, w=4, scale=8, grid=3, lsc=0.25, vsc=8.0)

    def call(**kw):
        a = {**ok, **kw}
        return lib.scflow_convex_upsample(a["logits"], a["ls"], a["lr"], a["delta"], a["occ"],
                                          a["flow_up"], a["occ_up"], a["next0"], a["s0"], a["next1"],
                                          a["s1"], a["n"], a["h"], a["w"], a["scale"], a["grid"],
                                          a["lsc"], a["vsc"], None)
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    for bad in (dict(logits=None), dict(lr=None), dict(flow_up=None), dict(occ_up=None), dict(n=0),
                dict(h=-1), dict(w=0), dict(ls=575), dict(s0=1), dict(s1=0), dict(scale=0),
                dict(grid=-3)):
        assert call(**bad) == EINVAL, bad
    for bad in (dict(scale=4), dict(scale=16), dict(grid=5), dict(grid=1)):
        assert call(**bad) == EUNSUPPORTED, bad
    for bad in (dict(flow_up=p + 4), dict(occ_up=p + 8)):
        assert call(**bad) == EALIGN, bad
    assert lib.scflow_flow_add(None, p, p, 2, None, 0, 1, 4, 4, None) == EINVAL
    assert lib.scflow_flow_add(p, p, p, 1, None, 0, 1, 4, 4, None) == EINVAL


def test_restated_upsampling_has_the_reference_channel_order():
    """One hot logit per (pixel, sub-pixel): the restatement must pick exactly that neighbour."""
    g = torch.Generator().manual_seed(3)
    N, h, w = 1, 3, 4
    x = torch.randn(N, 2, h, w, generator=g)
    pick = torch.randint(0, 9, (N, 64, h, w), generator=g)
    logits = torch.full((N, 9, 64, h, w), -4000.0)
    logits.scatter_(1, pick[:, None], 0.0)
    up = rr.convex_upsample(x, logits.view(N, 576, h, w), value_scale=8.0)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    for y in range(h):
        for xx in range(w):
            for s in (0, 9, 37, 63):
                ky, kx = divmod(int(pick[0, s, y, xx]), 3)
                want = 8.0 * xp[0, :, y + ky, xx + kx]
                got = up[0, :, 8 * y + s // 8, 8 * xx + s % 8]
                assert torch.equal(got, want), (y, xx, s)


def test_restatement_matches_reference_fixture():
    """The bounds tests/test_oracle_golden.py uses for the SCFlow fixture: upflow mean EPE ≤ 1e-3
    px, occlusion atol 1e-5 (and the low-resolution flow after every iteration, which localises a
    failure)."""
    g = rr.raft_golden()
    B, S, iters, in_seed, w_seed = (int(v) for v in g["meta"])
    inp = rr.raft_inputs(B, S, in_seed, g)
    out = rr.raft_forward(rr.raft_state_dict("mask", w_seed), **inp, iters=iters)
    for i in range(iters):
        np.testing.assert_allclose(out["lr_flow"][i].numpy(), g["lr_flow"][i], atol=1e-4)
    epe = rr.mean_epe(t(g["upflow_last"]), out["upflow"][-1])
    print(f"restatement vs reference: upflow mean EPE {epe:.3e} px")
    assert epe <= rr.EPE_TOL
    np.testing.assert_allclose(out["upocc"][-1].numpy(), g["upocclusion_last"], atol=1e-5)
    # RAFTDecoder: the same flow without the occlusion head
    plain = rr.raft_forward(rr.raft_state_dict("plain", w_seed), **inp, iters=iters, occlusion=False)
    assert plain["upocc"] == [] and rr.mean_epe(t(g["upflow_last"]), plain["upflow"][-1]) <= rr.EPE_TOL
