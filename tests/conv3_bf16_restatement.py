"""What the bf16 3×3 tests share (no tests here): the fp64 restatement of one launch of the bf16
direct 3×3 conv (SCFLOW_CONV_BF16_3X3) on rounded operands, and the oracle's MotionEncoder with
the operands the device rounds rounded — the "emulated oracle" the decoder tests install over
``oracle.scflow_oracle.motion_encoder``.

The kernel's contract ("bf16 motion-encoder convs"): out = act(Σ bf16(x)·bf16(w)
accumulated in fp32, + bias); bf16(·) is round-to-nearest-even of the fp32 value, products are
exact, so an fp64 evaluation on the rounded operands differs from the device by the summation
order only.
"""
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import scflow_oracle as orc
from tests import gru_bf16_restatement as gr
from tests.gru_bf16_restatement import round_bf16  # noqa: F401  (the tests take it from here)

ACTS = {None: lambda v: v, "ReLU": torch.relu, "Sigmoid": torch.sigmoid, "Tanh": torch.tanh}


def launch(src, weight, bias, act=None, rounded=True):
    """One launch over the NCHW fp32 ``src`` (both sources concatenated): fp64 3×3 "same" conv of
    the (rounded) source with the (rounded) OIHW fp32 ``weight``, plus the exact bias (may be
    None), then the activation."""
    rnd = round_bf16 if rounded else (lambda t: t)
    y = F.conv2d(rnd(src).double(), rnd(weight).double(), None if bias is None else bias.double(),
                 padding=1)
    return ACTS[act](y)


def _conv3_rounded(x, sd, prefix, act):
    """``orc.conv_module`` for a 3×3 "same" conv with its input and weight rounded to bf16."""
    w = round_bf16(sd[prefix + ".conv.weight"]).to(x.dtype)
    b = sd.get(prefix + ".conv.bias")
    return ACTS[act](F.conv2d(round_bf16(x), w, None if b is None else b.to(x.dtype), padding=1))


def motion_encoder_bf16(sd, corr, flow, act="ReLU", prefix="encoder"):
    """``oracle.scflow_oracle.motion_encoder`` with what ``MotionEncoder.bf16`` rounds rounded: the
    inputs and weights of corr_net.1, flow_net.1 and out_net.0.  corr_net.0 (1×1) and flow_net.0
    (7×7) stay exact, and so do the biases and the flow channels appended to the output."""
    c = orc.conv_module(corr, sd, f"{prefix}.corr_net.0", act, padding=0)
    c = _conv3_rounded(c, sd, f"{prefix}.corr_net.1", act)
    f = orc.conv_module(flow, sd, f"{prefix}.flow_net.0", act, padding=3)
    f = _conv3_rounded(f, sd, f"{prefix}.flow_net.1", act)
    o = _conv3_rounded(torch.cat([c, f], 1), sd, f"{prefix}.out_net.0", act)
    return torch.cat([o, flow], 1)


class emulating:
    """Context manager: ``orc.motion_encoder`` is the emulation for its duration, and with
    ``gru_cxt_channels`` not None ``orc.conv_gru`` is ``gr.emulated(gru_cxt_channels)`` too (both
    knobs); the oracle's own functions are put back on exit."""

    def __init__(self, gru_cxt_channels=None):
        self.gru = gru_cxt_channels

    def __enter__(self):
        self.saved = orc.motion_encoder, orc.conv_gru
        orc.motion_encoder = motion_encoder_bf16
        if self.gru is not None:
            orc.conv_gru = gr.emulated(self.gru)
        return self

    def __exit__(self, *exc):
        orc.motion_encoder, orc.conv_gru = self.saved
        return False


@lru_cache(maxsize=None)
def _fp32_case(B, S, seed, iters, w_seed, feat_size):
    """(inputs, decoder, its state dict on the CPU, fp32 oracle outputs) of one synthetic case:
    what ``oracle_pair`` shares between the emulations of one knob and of both."""
    from tests.helpers import decoder_inputs
    from tests.test_gpu_decoder import build_decoder
    inp = decoder_inputs(B, S, seed)
    dec = build_decoder(iters, feat_size=feat_size, seed=w_seed)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    return inp, dec, sd, orc.decoder_forward(sd, **inp, iters=iters)


@lru_cache(maxsize=None)
def oracle_pair(B, S, seed, iters, w_seed, with_gru=False, feat_size=None):
    """(inputs, decoder, fp32 oracle outputs, emulated oracle outputs) for one synthetic
    SCFlowDecoder case, computed once and shared; nothing in it may be modified.  The emulated
    oracle rounds the motion encoder's three 3×3 convs, and with ``with_gru`` the hoisted-context
    GRU convs as well (``decoder.menc_bf16`` and ``decoder.gru_bf16`` together)."""
    inp, dec, sd, ref = _fp32_case(B, S, seed, iters, w_seed, feat_size)
    with emulating(128 if with_gru else None):
        emu = orc.decoder_forward(sd, **inp, iters=iters)
    return inp, dec, ref, emu
