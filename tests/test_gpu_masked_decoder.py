"""GPU: SCFlowDecoder with occlusion masking (mask_flow / mask_corr, scflow_decoder.py:189-207)
on the fused schedule — parity against the fixture produced by the reference itself (B=2, 256², 4
iterations, both flags) and the CPU oracle (every flag combination, every iteration; 512² for the
64×64-map lookup), the plan taken (``SCFlowDecoder.last_plan``), bit-identity of the schedules
under masking, and a delayed side stream.  Bars as tests/test_gpu_decoder.py: EPE 1e-3 px,
rotations 1e-5, translations 1e-3, Δpose 1e-5, mask 1e-4.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests.helpers import decoder_inputs, t
from tests.test_gpu_decoder import EPE_TOL, build_decoder, check_against, run_gpu
from tests.test_masked_host import masked_e2e_fixture

pytestmark = pytest.mark.gpu
orc = pytest.importorskip("oracle.scflow_oracle")

FLAGS = [(True, False), (False, True), (True, True)]  # (mask_flow, mask_corr)


def masked_decoder(iters, flags=(True, True), **kw):
    dec = build_decoder(iters, **kw)
    dec.mask_flow, dec.mask_corr = flags
    return dec


def test_masked_decoder_matches_reference_golden():
    g = masked_e2e_fixture()
    B, S, iters, seed = (int(v) for v in g["meta"])
    inp = decoder_inputs(B, S, seed, g)
    dec = masked_decoder(iters)
    out = run_gpu(dec, inp)
    assert len(out) == 7 and all(len(l) == iters for l in out)
    check_against(out, t(g["flow_pose_last"]), t(g["flow_pred_last"]), g["R"], g["t"])
    np.testing.assert_allclose(torch.stack(out[5]).numpy(), g["drot"], atol=1e-5)
    np.testing.assert_allclose(torch.stack(out[6]).numpy(), g["dt"], atol=1e-5)
    np.testing.assert_allclose(out[4][-1].numpy(), g["mask_last"], atol=1e-4)
    assert dec.last_plan["fuse_tail"] and dec.last_plan["fuse_lc"]


@lru_cache(maxsize=None)
def _b4_inputs():
    return decoder_inputs(4, 256, seed=21)


@pytest.mark.parametrize("flags", FLAGS)
def test_masked_decoder_matches_oracle_b4(flags):
    """B=4, 256², 4 iterations: every iteration against the oracle with the same flags."""
    inp = _b4_inputs()
    dec = masked_decoder(4, flags, seed=1)
    out = run_gpu(dec, inp)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=4, mask_flow=flags[0], mask_corr=flags[1])
    check_against(out, ref[0][-1], ref[1][-1], torch.stack(ref[2]).numpy(), torch.stack(ref[3]).numpy())
    for i in range(4):
        for k in (0, 1):
            epe = float(orc.cal_epe_mean(ref[k][i], out[k][i]).max())
            print(f"flags {flags} iteration {i} list {k}: EPE {epe:.3e}")
            assert epe <= EPE_TOL


def test_masked_decoder_512_feat64():
    """B=1, 512² (64×64 maps): the tile-row lookup, no fused 1×1."""
    inp = decoder_inputs(1, 512, seed=5)
    dec = masked_decoder(2, feat_size=(64, 64), seed=2)
    out = run_gpu(dec, inp)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=2, mask_flow=True, mask_corr=True)
    check_against(out, ref[0][-1], ref[1][-1])
    assert not dec.last_plan["fuse_lc"]


def test_masked_decoder_takes_the_unmasked_plan():
    inp = decoder_inputs(2, 256, seed=13)
    plain = build_decoder(3, seed=4)
    assert plain.last_plan is None
    run_gpu(plain, inp)
    want = plain.last_plan
    assert want["fuse_tail"] and want["fuse_lc"] and want["pair_tail"] and want["defer"]
    for flags in FLAGS:
        dec = masked_decoder(3, flags, seed=4)
        run_gpu(dec, inp)
        assert dec.last_plan == want, flags
    got = dec.last_plan
    got["fuse_tail"] = False  # a copy: the decoder's record is read-only
    assert dec.last_plan == want


def _equal_lists(a, b, what):
    for la, lb in zip(a, b):
        for x, y in zip(la, lb):
            assert torch.equal(x, y), what


def test_masked_decoder_schedules_bit_identical():
    """Under both flags every schedule gives the default plan's bits on all seven lists: fused
    tail on / off, fused lookup + 1×1 on / off, paired tail 0 / 1, side stream on / off, deferred
    full-resolution outputs on / off, default events.  The fused masked kernels against the plain
    composition (masked lookup → 1×1 conv, masked downsample → separate tail launches), end to
    end."""
    inp = decoder_inputs(2, 256, seed=13)
    dec = masked_decoder(3, seed=4)
    base = run_gpu(dec, inp)
    default = dict(fuse_tail=True, fuse_lookup_conv=True, pair_tail=-1, side_stream=True,
                   defer_full_res=True, device_scope_events=True)
    variants = [dict(fuse_tail=False), dict(fuse_lookup_conv=False), dict(pair_tail=0),
                dict(pair_tail=1), dict(side_stream=False), dict(defer_full_res=False),
                dict(device_scope_events=False), dict(fuse_tail=False, side_stream=False),
                dict(fuse_tail=False, pair_tail=0, fuse_lookup_conv=False),
                dict(defer_full_res=False, pair_tail=0)]
    for v in variants:
        for k, val in {**default, **v}.items():
            assert hasattr(dec, k), k
            setattr(dec, k, val)
        out = run_gpu(dec, inp)
        for k in ("fuse_tail", "fuse_lookup_conv"):
            assert dec.last_plan["fuse_lc" if k == "fuse_lookup_conv" else k] == {**default, **v}[k]
        _equal_lists(base, out, v)
    # and the flags do change the result (the masks of the synthetic weights are not saturated)
    plain = run_gpu(build_decoder(3, seed=4), inp)
    assert not torch.equal(plain[0][-1], base[0][-1])


@pytest.mark.parametrize("flags", [(False, False), (True, True)])
def test_masked_decoder_side_stream_delay(flags):
    """The default plan, unmasked and with both mask flags, with every deferred full-resolution
    launch held back on the side stream by ordinary work queued right before it (the "pose_flow"
    hook fires there: two large correlation pyramids on scratch inputs, milliseconds) while the
    main stream runs on into the next pose step: the same bits as the undelayed run — every
    buffer a deferred launch reads is ordered against its next writer by an event or is a buffer
    of its own.  (The unmasked case also passed before the unmasked plan had its mark / wait:
    the delaying GEMMs fill every CU, so the main stream does not get far ahead of them either.
    That ordering rests on the code and tests/test_decoder_streams.py.)"""
    from scflow_amd import ops
    inp = decoder_inputs(2, 256, seed=13)
    dec = masked_decoder(4, flags, seed=4).cuda()
    base = run_gpu(dec, inp)
    assert dec.last_plan["side_stream"] and dec.last_plan["defer"] and dec.last_plan["pair_tail"]
    dev = torch.device("cuda", torch.cuda.current_device())
    side = dec._side_stream(dev, 0)
    g = torch.Generator().manual_seed(3)
    f1 = torch.randn(8, 256, 64, 64, generator=g).cuda()
    f2 = torch.randn(8, 256, 64, 64, generator=g).cuda()
    torch.cuda.synchronize()
    fired = []

    def delay(start):
        if start:
            fired.append(torch.cuda.current_stream(dev) == side)
            for _ in range(2):
                ops.corr_pyramid(f1, f2, 4)

    dec.kernel_hooks["pose_flow"] = delay
    try:
        out = run_gpu(dec, inp)
    finally:
        dec.kernel_hooks.clear()
    # on the side stream before each deferred launch (iterations 0-2); the last iteration's whole
    # pose step carries the same hook on the main stream
    assert fired == [True] * 3 + [False]
    assert dec.last_plan["side_stream"] and dec.last_plan["defer"] and dec.last_plan["pair_tail"]
    _equal_lists(base, out, f"delayed side stream, flags {flags}")
