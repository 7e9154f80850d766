"""The core SCFlowDecoder and the RAFT decoders share (scflow_amd/recurrent.py) and the refiners'
shared base: the tiled / fused-lookup planning on the CPU for each decoder class, the refiner
families resolving the shared methods to one function, and on the GPU the two decoders' iteration
up to the GRU writing the same bits."""
import pytest
import torch

from tests import raft_restatement as rr
from tests.helpers import decoder_inputs

KINDS = ["SCFlowDecoder", "RAFTDecoder", "RAFTDecoderMask"]


def build(kind, iters=1, align_corners=True):
    from scflow_amd import MODELS
    if kind == "SCFlowDecoder":
        from tests.test_gpu_decoder import decoder_cfg
        cfg = decoder_cfg(iters)
    else:
        cfg = rr.raft_decoder_cfg(iters)
    cfg["corr_lookup_cfg"] = dict(align_corners=align_corners)
    return MODELS.build(dict(type=kind, **cfg)).eval()


@pytest.mark.parametrize("kind", KINDS)
def test_correlation_plan(kind):
    """(tiled, fuse_lc) as ops.tiled_pyramid_ok, ops.tiled_lookup_ok and ops.lookup_conv1x1_ok
    give them for 4 levels, radius 4 and the 1×1 324→256 corr_net.0."""
    from scflow_amd.recurrent import _RecurrentDecoder, plan_correlation
    dec = build(kind)
    assert isinstance(dec, _RecurrentDecoder)
    assert dec.plan_correlation(32, 32) == (True, True)
    assert dec.plan_correlation(64, 64) == (True, False)  # over fuse_lookup_conv_max_px
    assert dec.plan_correlation(40, 40) == (False, False)  # 40 % 32 != 0: no tiles, so no fusion
    dec.fuse_lookup_conv = False
    assert dec.plan_correlation(32, 32) == (True, False)
    dec.fuse_lookup_conv, dec.tiled_pyramid = True, False
    assert dec.plan_correlation(32, 32) == (False, False)
    # without align_corners: every level is at least 9 wide or held whole, so tiled stays
    assert build(kind, align_corners=False).plan_correlation(32, 32)[0] is True
    # the method is the pure function with the decoder's knobs
    dec.tiled_pyramid = True
    assert plan_correlation(True, True, 32 * 32, dec.encoder.corr_net, 32, 32, 4, 4, True) == \
        dec.plan_correlation(32, 32) == (True, True)
    assert plan_correlation(True, True, 16 * 16, dec.encoder.corr_net, 32, 32, 4, 4, True) == \
        (True, False)


def test_decoders_share_one_base():
    from scflow_amd.decoder import SCFlowDecoder
    from scflow_amd.raft_decoder import RAFTDecoder, RAFTDecoderMask
    from scflow_amd.recurrent import _RecurrentDecoder
    for cls in (SCFlowDecoder, RAFTDecoder, RAFTDecoderMask):
        assert cls.hx_channels is _RecurrentDecoder.hx_channels
        assert cls.last_plan is _RecurrentDecoder.last_plan
        assert cls.plan_correlation is _RecurrentDecoder.plan_correlation
        assert cls.make_gru_block is _RecurrentDecoder.make_gru_block
    assert RAFTDecoder._hidden_heads is _RecurrentDecoder._hidden_heads
    dec = build("SCFlowDecoder")
    assert dec._hidden_heads() is dec._hidden_heads()  # the no-argument wrapper, cached runner
    assert dec._hidden_heads() is _RecurrentDecoder._hidden_heads(
        dec, (("flow", dec.flow_pred), ("mask", dec.mask_pred)))


def test_refiners_share_one_base():
    from scflow_amd.raft_refiner import RAFTRefinerFlow, RAFTRefinerFlowMask
    from scflow_amd.refiner import SCFlowRefiner, _RefinerBase
    for cls in (SCFlowRefiner, RAFTRefinerFlow, RAFTRefinerFlowMask):
        assert issubclass(cls, _RefinerBase)
        assert cls.extract_feat is _RefinerBase.extract_feat
        assert cls._features_into_hx is _RefinerBase._features_into_hx
        assert cls.freeze_bn is _RefinerBase.freeze_bn


@pytest.mark.gpu
def test_decoders_run_one_core():
    """SCFlowDecoder and RAFTDecoderMask with the same encoder / GRU weights, features, zero flow
    and identically filled hx buffers: after one iteration the new hidden state, the context and
    the motion features are the same bits, on the fused path and on the separate-lookup path."""
    from scflow_amd import synthetic
    sc, raft = build("SCFlowDecoder"), build("RAFTDecoderMask")
    synthetic.fill_module_(sc, seed=0)
    shared = {k: v for k, v in sc.state_dict().items() if k.startswith(("encoder.", "gru."))}
    assert shared and not raft.load_state_dict(shared, strict=False).unexpected_keys
    sc, raft = sc.cuda(), raft.cuda()
    inp = {k: v.cuda() for k, v in decoder_inputs(2, 256, seed=3).items()}
    N, _, h, w = inp["feat_render"].shape
    assert (h, w) == (32, 32)
    keep = sc.h_channels + sc.cxt_channels + sc.encoder.out_channels[0]
    assert sc.hx_channels == raft.hx_channels == keep + 2
    hx0 = torch.tanh(torch.randn(N * h * w, sc.hx_channels, generator=torch.Generator().manual_seed(1)))
    for fused in (True, False):
        for dec in (sc, raft):
            dec.fuse_lookup_conv = dec.tiled_pyramid = fused
        hx_sc, hx_raft = hx0.cuda(), hx0.cuda()
        with torch.no_grad():
            sc._forward(inp["feat_render"], inp["feat_real"], None, None, inp["ref_rotation"],
                        inp["ref_translation"], inp["depth"], inp["internel_k"], inp["label"],
                        torch.zeros_like(inp["init_flow"]), 0.0, hx=hx_sc)
            raft._forward(inp["feat_render"], inp["feat_real"], torch.zeros(N, 2, h, w, device="cuda"),
                          None, None, hx=hx_raft)
        torch.cuda.synchronize()
        assert sc.last_plan["fuse_lc"] == raft.last_plan["fuse_lc"] == fused
        assert sc.last_plan["tiled"] == raft.last_plan["tiled"] == fused
        assert not torch.equal(hx_sc[:, :sc.h_channels], hx0[:, :sc.h_channels].cuda())  # it ran
        assert torch.equal(hx_sc[:, :keep], hx_raft[:, :keep]), f"fused={fused}"
