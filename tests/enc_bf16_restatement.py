"""What the bf16 encoder tests share (no tests here): the fp64 restatement of one launch of the
bf16 direct 3×3 conv in its RAFT-encoder form (SCFLOW_CONV_BF16_3X3N) on rounded operands, the
stages ``RAFTEncoder.bf16`` is wired to, and the oracle's BasicBlock with the operands the device
rounds rounded — the "emulated oracle" the encoder and refiner tests install over
``oracle.scflow_oracle._basic_block``.

The kernel's contract: x' = relu(fmaf(x, in_scale[img][c], in_shift[img][c])) — one
fp32 rounding — when both are given, else x' = x; zero padding pads x'; y = Σ bf16(x')·bf16(w)
accumulated in fp32; v = y + bias; v = v·out_scale[o] + out_shift[o] if given; v += res if given;
out = act(v).  An fp64 evaluation on the rounded operands differs from the device by the summation
order and the epilogue's fp32 roundings only.
"""
import re
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import scflow_oracle as orc
from tests.conv3_bf16_restatement import ACTS
from tests.gru_bf16_restatement import round_bf16

# the stages whose stride-1 3×3 convs the knob runs in bf16 (scflow_amd.encoder.BF16_STAGES, by the
# wiring table of DESIGN.md §26; the host test holds the two together)
WIRED = ("res_layer1", "res_layer2", "res_layer3")


def launch(x, weight, bias, in_scale=None, in_shift=None, out_scale=None, out_shift=None, res=None,
           act=None, rounded=True):
    """One launch over the NCHW fp32 ``x``: fp64.  in_scale / in_shift [n][c], out_scale /
    out_shift [cout], res NCHW; ``rounded`` False leaves x' and the weights unrounded (the negative
    control)."""
    rnd = round_bf16 if rounded else (lambda t: t)
    if in_scale is not None:
        sc, sh = in_scale.double()[:, :, None, None], in_shift.double()[:, :, None, None]
        x = torch.relu((x.double() * sc + sh).float())
    v = F.conv2d(rnd(x).double(), rnd(weight).double(), None if bias is None else bias.double(),
                 padding=1)
    if out_scale is not None:
        v = v * out_scale.double()[None, :, None, None] + out_shift.double()[None, :, None, None]
    if res is not None:
        v = v + res.double()
    return ACTS[act](v)


def _stage(p):
    m = re.search(r"(res_layer\d+)\.\d+\.$", p)
    return m.group(1) if m else None


def basic_block_bf16(sd, p, x, stride, norm, train=False):
    """``oracle.scflow_oracle._basic_block`` with what ``RAFTEncoder.bf16`` rounds rounded: in a
    wired stage the input and the weight of conv1 when its stride is 1, and of conv2 — whose input
    is the normalised, rectified conv1 output, which the device rounds after the fused IN + ReLU
    (or reads back, in the BN form, from conv1's epilogue).  Biases, norms, the downsample branch
    and the identity stay exact."""
    if _stage(p) not in WIRED:
        return _plain_basic_block(sd, p, x, stride, norm, train)
    ab = "in" if norm == "IN" else "bn"
    if stride == 1:
        out = F.conv2d(round_bf16(x), round_bf16(sd[p + "conv1.weight"]), sd[p + "conv1.bias"], padding=1)
    else:
        out = F.conv2d(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"], stride=stride, padding=1)
    out = F.relu(orc._enc_norm(out, sd, p + ab + "1", norm, train=train))
    out = F.conv2d(round_bf16(out), round_bf16(sd[p + "conv2.weight"]), sd[p + "conv2.bias"], padding=1)
    out = orc._enc_norm(out, sd, p + ab + "2", norm, train=train)
    if p + "downsample.0.weight" in sd:
        identity = F.conv2d(x, sd[p + "downsample.0.weight"], sd[p + "downsample.0.bias"], stride=stride)
        identity = orc._enc_norm(identity, sd, p + "downsample.1", norm, train=train)
    else:
        identity = x
    return F.relu(out + identity)


_plain_basic_block = orc._basic_block  # the oracle's own, taken before anything is installed


class emulating:
    """Context manager: ``orc._basic_block`` is the emulation for its duration; the oracle's own
    function is put back on exit.  Nests with the decoder knobs' ``emulating``."""

    def __enter__(self):
        self.saved = orc._basic_block
        orc._basic_block = basic_block_bf16
        return self

    def __exit__(self, *exc):
        orc._basic_block = self.saved
        return False


def wired_convs(blocks=(2, 2, 2), strides=(1, 2, 2)):
    """The conv names ``last_bf16`` lists for a 'Basic' encoder with the knob on."""
    out = []
    for i, (nb, s) in enumerate(zip(blocks, strides)):
        name = f"res_layer{i + 1}"
        if name not in WIRED:
            continue
        for b in range(nb):
            if b > 0 or s == 1:
                out.append(f"{name}.{b}.conv1")
            out.append(f"{name}.{b}.conv2")
    return tuple(out)


# ---------------------------------------------------------------------------------- shared oracles
@lru_cache(maxsize=None)
def encoder_pair(norm, seed, B, S, img_seed=21):
    """(images, fp32 oracle features, emulated oracle features) of one encoder case, computed once
    and shared; nothing in it may be modified."""
    from scflow_amd import synthetic
    from tests.helpers import encoder_state_dict, t
    x = t(synthetic.make_images(B, S, seed=img_seed)["real_images"])
    sd = encoder_state_dict(norm, seed)
    ref = orc.raft_encoder(sd, x, norm)
    with emulating():
        emu = orc.raft_encoder(sd, x, norm)
    return x, ref, emu


def get_pose(sd, inp, iters):
    """The oracle's SCFlowRefiner.get_pose: extract_feat, then the decoder from a zero flow."""
    render, real, h, c = orc.extract_feat(sd, inp["render_images"], inp["real_images"])
    N, H, W = inp["depth"].shape
    return orc.decoder_forward(sd, render, real, h, c, inp["ref_rotation"], inp["ref_translation"],
                               inp["depth"], inp["internel_k"], inp["label"],
                               torch.zeros(N, 2, H, W), iters=iters)


@lru_cache(maxsize=None)
def refine_pair():
    """(inputs, iterations, fp32 oracle outputs, outputs emulating ``enc_bf16`` alone, outputs
    emulating all three knobs) on the refine golden's inputs, computed once and shared."""
    from tests import conv3_bf16_restatement as cr
    from tests.helpers import golden, refine_inputs, refiner_state_dict
    g = golden("refine")
    B, S, iters, seed = (int(v) for v in g["meta"])
    inp = refine_inputs(B, S, seed, g)
    sd = refiner_state_dict()
    ref = get_pose(sd, inp, iters)
    with emulating():
        enc = get_pose(sd, inp, iters)
        with cr.emulating(128):
            three = get_pose(sd, inp, iters)
    return inp, iters, ref, enc, three
