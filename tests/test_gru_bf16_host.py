"""CPU: the opt-in bf16 GRU conv (SCFLOW_CONV_BF16) as far as it goes without a device — the
rounding restatement the GPU tests lean on, the launch plan through the host-only
scflow_conv_plan_kind (fake aligned pointers, nothing launched), the packed size, the Python knobs
and the emulated oracle.  On the parent commit format 6 is SCFLOW_EINVAL and the knobs do not exist."""
import ctypes

import pytest
import torch

from scflow_amd import _lib, ops
from tests import gru_bf16_restatement as gr

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
SRC0, SRC1, WEIGHT, OUT, GATE, RH, HID, BMAP = (0x10000 * (i + 1) for i in range(8))
EPI = {"plain": dict(epilogue=_lib.EPI_PLAIN),
       "zr": dict(epilogue=_lib.EPI_GRU_ZR, gate=GATE, rh=RH, hid=HID, out=None),
       "q": dict(epilogue=_lib.EPI_GRU_Q, gate=GATE, hid=HID, out=None)}
GRU_SPLITS = [(128, 128), (384, 0), (128, 256)]  # hoisted z|r and q; full-width z|r; full-width q


def conv(n, h, w, c0, c1, cout, k, bk=None, **over):
    kh, kw = (k, k) if isinstance(k, int) else k
    a = _lib.ConvArgs()
    a.src0, a.c0, a.s0 = SRC0, c0, c0
    if c1:
        a.src1, a.c1, a.s1 = SRC1, c1, c1
    a.weight, a.out, a.so = WEIGHT, OUT, cout
    a.n, a.h, a.w, a.cout = n, h, w, cout
    a.kh, a.kw, a.ph, a.pw, a.stride = kh, kw, kh // 2, kw // 2, 1
    a.gate, a.sg, a.rh, a.srh, a.hid, a.sh = None, 128, None, 128, None, 128
    a.bk = _lib.CONV_BF16 if bk is None else bk
    for key, v in over.items():
        setattr(a, key, v)
    return a


def kind(a, b=None):
    k = ctypes.c_int(-7)
    status = _lib.load().scflow_conv_plan_kind(ctypes.byref(a), ctypes.byref(b) if b is not None else None,
                                               ctypes.byref(k))
    return status, k.value


# ------------------------------------------------------------------------------------- rounding
def test_round_bf16_matches_torch_on_random_values():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(1 << 16, generator=g),
                   torch.randn(1 << 12, generator=g) * 1e-30,
                   torch.randn(1 << 12, generator=g) * 1e30,
                   torch.randint(-8, 9, (256,), generator=g).float()])
    assert torch.equal(gr.round_bf16(x), x.bfloat16().float())
    assert gr.round_bf16(x.double()).dtype == torch.float64


def test_round_bf16_ties_go_to_even():
    big = float(torch.finfo(torch.bfloat16).max)  # 0x7f7f0000
    below_tie = torch.tensor(0x7F7F7FFF, dtype=torch.int32).view(torch.float32).item()
    cases = [(1 + 2 ** -8, 1.0),               # tie, kept part even: down
             (1 + 3 * 2 ** -8, 1 + 2 ** -6),   # tie, kept part odd: up
             (1 + 2 ** -8 + 2 ** -20, 1 + 2 ** -7),  # above the tie
             (1 + 2 ** -8 - 2 ** -20, 1.0),    # below the tie
             (-(1 + 2 ** -8), -1.0), (-(1 + 3 * 2 ** -8), -(1 + 2 ** -6)),
             (big, big), (-big, -big), (below_tie, big), (-below_tie, -big),
             (0.0, 0.0), (0.5, 0.5), (-0.25, -0.25)]
    x = torch.tensor([c[0] for c in cases], dtype=torch.float32)
    want = torch.tensor([c[1] for c in cases], dtype=torch.float32)
    assert torch.equal(gr.round_bf16(x), want)
    assert torch.equal(x.bfloat16().float(), want)


# ------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("c0,c1", GRU_SPLITS)
@pytest.mark.parametrize("k", [(1, 5), (5, 1)])
@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("epi", ["plain", "zr", "q"])
def test_gru_shapes_plan_the_bf16_kernel(c0, c1, k, w, epi):
    cout = 256 if epi == "zr" else 128
    for n in (1, 16):
        assert kind(conv(n, w, w, c0, c1, cout, k, **EPI[epi])) == (OK, _lib.PLAN_SEP_BF16)
    assert kind(conv(1, 4, w, c0, c1, cout, k, **EPI[epi])) == (OK, _lib.PLAN_SEP_BF16)


def test_outside_the_domain_is_unsupported():
    refused = (EUNSUPPORTED, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 128, 128, 3)) == refused                    # 3×3
    assert kind(conv(2, 32, 32, 128, 128, 128, (1, 5), stride=2)) == refused     # stride 2
    assert kind(conv(2, 48, 48, 128, 128, 128, (1, 5))) == refused               # W = 48
    assert kind(conv(2, 32, 32, 130, 0, 128, (1, 5))) == refused                 # c0 = 130
    assert kind(conv(2, 32, 32, 132, 0, 128, (1, 5))) == refused                 # c0 % 32
    assert kind(conv(2, 32, 32, 128, 16, 128, (1, 5))) == refused                # c1 % 32
    assert kind(conv(2, 32, 32, 128, 128, 48, (1, 5))) == refused                # cout = 48
    assert kind(conv(2, 32, 32, 128, 0, 128, (1, 5), in_scale=BMAP, in_shift=BMAP)) == refused
    assert kind(conv(2, 32, 32, 128, 0, 128, (1, 5), res=BMAP, sres=128)) == refused
    assert kind(conv(2, 32, 32, 128, 128, 128, (1, 5), pw=1)) == refused         # not "same"
    assert kind(conv(2, 6, 32, 128, 128, 128, (5, 1))) == refused                # 5×1: h % 4
    assert kind(conv(2, 31, 64, 128, 128, 128, (1, 5))) == refused               # 1×5, W 64: h % 2
    # the format's own alignment and argument checks
    assert kind(conv(2, 32, 32, 128, 128, 128, (1, 5), s0=386)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 128, 128, (1, 5), out=None)) == (EINVAL, _lib.PLAN_NONE)
    a = conv(2, 32, 32, 128, 128, 128, 3)
    assert _lib.load().scflow_conv_workspace_bytes(ctypes.byref(a)) == EUNSUPPORTED
    a = conv(2, 32, 32, 128, 128, 128, (1, 5))
    assert _lib.load().scflow_conv_workspace_bytes(ctypes.byref(a)) == 0


def test_source_1s_stride_counts_only_when_it_has_channels():
    """With c1 == 0 every stage is source 0's and the kernel never reads source 1: whatever s1
    holds — unaligned, or large enough to push the offset bound past the buffer-load range — the
    launch plans, as it does for the 3×3 formats."""
    for s1 in (0, 3, 1 << 30):
        for k in ((1, 5), (5, 1)):
            assert kind(conv(2, 32, 32, 256, 0, 128, k, s1=s1)) == (OK, _lib.PLAN_SEP_BF16)
    # with channels it counts as before
    assert kind(conv(2, 32, 32, 128, 128, 128, (1, 5), s1=1 << 30)) == (EUNSUPPORTED, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 128, 128, (1, 5), s1=64)) == (EUNSUPPORTED, _lib.PLAN_NONE)


def test_a_pair_with_a_bf16_half_is_two_launches():
    a = conv(2, 32, 32, 128, 128, 256, (1, 5), **EPI["zr"])
    for b in (conv(2, 32, 32, 128, 128, 128, (1, 5)),                     # bf16 beside bf16
              conv(2, 32, 32, 128, 0, 64, 3, bk=_lib.CONV_WINO),          # beside F(2×2,3×3)
              conv(2, 32, 32, 256, 0, 1, 1, bk=16)):                      # beside a thin conv
        assert kind(a, b) == (OK, _lib.PAIR_NONE) and kind(b, a) == (OK, _lib.PAIR_NONE)
    bad = conv(2, 32, 32, 130, 0, 128, (1, 5))
    assert kind(a, bad) == (EUNSUPPORTED, _lib.PAIR_NONE)


@pytest.mark.parametrize("c0,c1", GRU_SPLITS)
@pytest.mark.parametrize("k,pad", [((1, 5), (0, 2)), ((5, 1), (2, 0))])
def test_the_default_format_is_unchanged(c0, c1, k, pad):
    for n, s in ((1, 32), (16, 32), (1, 64), (32, 64)):
        for cout in (128, 256):
            assert ops.conv_pick_bk(n, s, s, c0, c1, cout, *k, *pad) == _lib.CONV_WINO


def test_packed_size_is_the_headers_formula():
    size = _lib.load().scflow_conv_packed_size_bk
    for cout, c0, c1 in [(256, 128, 128), (256, 384, 0), (128, 128, 256), (96, 64, 32), (32, 32, 0)]:
        for k in ((1, 5), (5, 1)):
            for w in (32, 64):
                want = (cout + 63) // 64 * 64 * (c0 + c1) * 5 // 2  # two bf16 per float
                assert size(cout, c0, c1, *k, 1, w, _lib.CONV_BF16) == want
    assert size(128, 128, 128, 3, 3, 1, 32, _lib.CONV_BF16) == EUNSUPPORTED
    assert size(128, 130, 0, 1, 5, 1, 32, _lib.CONV_BF16) == EUNSUPPORTED
    assert size(128, 128, 0, 1, 5, 1, 48, _lib.CONV_BF16) == EUNSUPPORTED
    assert size(128, 128, 0, 1, 5, 1, 32, 5) == EINVAL  # 5 stays no format


def test_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "scflow_hip.h")).read()
    assert int(re.search(r"#define SCFLOW_CONV_BF16 (\d+)", hdr).group(1)) == _lib.CONV_BF16 == 6
    assert int(re.search(r"#define SCFLOW_PLAN_SEP_BF16 (\d+)", hdr).group(1)) == _lib.PLAN_SEP_BF16 == 14


# ------------------------------------------------------------------------------------- the knobs
def test_conv_gru_flag_picks_the_runners_format():
    from scflow_amd.modules import ConvGRU
    gru = ConvGRU(128, 256, "SeqConv")
    assert gru.bf16 is False
    assert all(r.fmt is None for pair in gru.runners() for r in pair)
    assert all(r.fmt is None for trio in gru._ctx_runners(128) for r in trio)
    gru.bf16 = True
    assert all(r.fmt == _lib.CONV_BF16 for pair in gru.runners() for r in pair)
    for rzr, rq, rctx in gru._ctx_runners(128):
        assert rzr.fmt == _lib.CONV_BF16 and rq.fmt == _lib.CONV_BF16
        assert rctx.fmt is None  # the hoisted-context conv keeps the library's fp32 choice
    gru.bf16 = False
    assert all(r.fmt is None for pair in gru.runners() for r in pair)
    assert all(r.fmt is None for trio in gru._ctx_runners(128) for r in trio)


def test_a_runner_with_a_format_does_not_ask_the_library(monkeypatch):
    from scflow_amd.modules import ConvRunner
    r = ConvRunner([torch.nn.Conv2d(256, 128, (1, 5), padding=(0, 2))], "Tanh")
    assert r._pick(2, 32, 32, 128, 128) == _lib.CONV_WINO
    r.fmt = _lib.CONV_BF16
    monkeypatch.setattr(ops, "conv_pick_bk", lambda *a, **k: pytest.fail("asked the library"))
    assert r._pick(2, 32, 32, 128, 128) == _lib.CONV_BF16
    monkeypatch.undo()
    r.fmt = None
    assert r._pick(2, 32, 32, 128, 128) == _lib.CONV_WINO


def test_decoders_default_to_fp32():
    from scflow_amd.recurrent import _RecurrentDecoder
    from tests import raft_restatement as rr
    from tests.test_gpu_decoder import build_decoder
    for dec in (build_decoder(2), rr.build_raft_decoder("RAFTDecoder", 2),
                rr.build_raft_decoder("RAFTDecoderMask", 2)):
        assert isinstance(dec, _RecurrentDecoder)
        assert dec.gru_bf16 is False and dec.gru.bf16 is False


# ------------------------------------------------------------------------------------- the oracle
def test_emulated_oracle_is_finite_and_differs_from_fp32():
    """The decoder test's yardstick at its shape (B = 2, 256², 4 iterations, synthetic weights):
    D_ref > 0 for every output family — the rounding moves every output the test looks at."""
    _, _, ref, emu = gr.oracle_pair(2, 256, 31, 4, 5, 128)
    for lst in emu:
        assert all(torch.isfinite(v).all() for v in lst)
    d = gr.distances(emu, ref)
    print("D_ref", d)
    assert all(d[f] > 0 for f in gr.FAMILIES), d


def test_emulation_rounds_only_what_the_device_rounds():
    """With exactly representable operands the emulation is the oracle's conv_gru bit for bit;
    the context channels and their weights are left exact when hoisted, rounded when not."""
    from oracle import scflow_oracle as orc
    g = torch.Generator().manual_seed(7)
    shapes = {f"gru.conv_{n}.{i}.conv.weight": (8, 24, *k) for n in "zrq"
              for i, k in enumerate([(1, 5), (5, 1)])}
    sd = {k: gr.round_bf16(torch.randn(s, generator=g) * 0.1) for k, s in shapes.items()}
    sd.update({k.replace("weight", "bias"): torch.randn(8, generator=g) * 0.1 for k in shapes})
    h = torch.tanh(torch.randn(1, 8, 8, 8, generator=g))
    x = torch.randn(1, 16, 8, 8, generator=g)
    # rounding changes the result, and the hoisted and un-hoisted emulations differ
    a, b, c = orc.conv_gru(sd, h, x), gr.conv_gru_bf16(sd, h, x, 8), gr.conv_gru_bf16(sd, h, x, 0)
    assert not torch.equal(a, b) and not torch.equal(b, c)
    # context weights a 16th of a bf16 half-ulp off their bf16 values: seen only where the
    # context is kept exact, rounded away where it is not
    sd2 = dict(sd)
    for k in shapes:
        w = sd[k].clone()
        w[:, 8:16] *= 1 + 2 ** -13
        sd2[k] = w
    assert not torch.equal(gr.conv_gru_bf16(sd2, h, x, 8), b)
    assert torch.equal(gr.conv_gru_bf16(sd2, h, x, 0), c)
