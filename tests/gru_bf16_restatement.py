"""What the bf16 GRU tests share (no tests here): bf16 rounding restated on the fp32 bits, the
fp64 restatement of one z|r launch and one q launch of the bf16 direct conv (SCFLOW_CONV_BF16) on
rounded operands, and the oracle's ConvGRU with the operands the device rounds rounded — the
"emulated oracle" the decoder tests install over ``oracle.scflow_oracle.conv_gru``.

The kernel's contract ("bf16 GRU convs"): out = epilogue(Σ bf16(x)·bf16(w) accumulated
in fp32, + bias + bias_map); bf16(·) is round-to-nearest-even of the fp32 value, products are exact,
so an fp64 evaluation on the rounded operands differs from the device by the summation order only.
"""
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import scflow_oracle as orc


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 values rounded to the nearest bf16 (ties to even), returned in ``t``'s dtype: integer
    arithmetic on the fp32 bits, add 0x7fff + the kept part's last bit, clear the low half.
    (Finite inputs; past bf16's largest finite the carry gives ±inf, as the hardware does.)"""
    u = t.detach().float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32).to(t.dtype)


def _rnd(t, on):
    return round_bf16(t) if on else t


def pre_activation(src, weight, bias, bias_map, pad, rounded=True):
    """fp64 conv of the (rounded) NCHW fp32 ``src`` with the (rounded) OIHW fp32 ``weight``, plus
    the exact bias and bias map (either may be None)."""
    y = F.conv2d(_rnd(src, rounded).double(), _rnd(weight, rounded).double(),
                 None if bias is None else bias.double(), padding=pad)
    return y if bias_map is None else y + bias_map.double()


def zr_launch(h, x, weight, bias, bias_map, pad, rounded=True):
    """One SCFLOW_EPI_GRU_ZR launch over cat[h, x] (NCHW fp32): fp64 (z, r·h); h in the product
    r·h is the exact fp32 hidden state (the epilogue reads it unrounded)."""
    hc = h.shape[1]
    pre = pre_activation(torch.cat([h, x], 1), weight, bias, bias_map, pad, rounded)
    return torch.sigmoid(pre[:, :hc]), torch.sigmoid(pre[:, hc:]) * h.double()


def q_launch(rh, x, weight, bias, bias_map, z, h, pad, rounded=True):
    """One SCFLOW_EPI_GRU_Q launch over cat[r·h, x]: fp64 (1 − z)·h + z·tanh(q), from the ``rh``
    and ``z`` the launch read (the device's own, so each launch is checked on the bits it read)."""
    q = torch.tanh(pre_activation(torch.cat([rh, x], 1), weight, bias, bias_map, pad, rounded))
    return (1 - z.double()) * h.double() + z.double() * q


def conv_gru_bf16(sd, h, x, cxt_channels, net_type="SeqConv", prefix="gru"):
    """``oracle.scflow_oracle.conv_gru`` with what ``ConvGRU.bf16`` rounds rounded: h (r·h for the
    q conv), the channels of x past the first ``cxt_channels`` and the matching weight columns.
    The context channels and their weight columns stay exact — the hoisted-context conv runs in
    fp32 (``cxt_channels=0``: everything is rounded, as with ``hoist_context=False``)."""
    prefix = prefix + "." if prefix else ""
    hc = h.shape[1]

    def conv(inp, name, i, act, pad):
        w = sd[f"{prefix}{name}.{i}.conv.weight"].to(inp.dtype).clone()
        w[:, :hc] = round_bf16(w[:, :hc])
        w[:, hc + cxt_channels:] = round_bf16(w[:, hc + cxt_channels:])
        b = sd.get(f"{prefix}{name}.{i}.conv.bias")
        y = F.conv2d(inp, w, None if b is None else b.to(inp.dtype), padding=pad)
        return torch.sigmoid(y) if act == "Sigmoid" else torch.tanh(y)

    xr = torch.cat([x[:, :cxt_channels], round_bf16(x[:, cxt_channels:])], 1)
    for i, (_, pad) in enumerate(orc.GRU_KERNELS[net_type]):
        hx = torch.cat([round_bf16(h), xr], 1)
        z = conv(hx, "conv_z", i, "Sigmoid", pad)
        r = conv(hx, "conv_r", i, "Sigmoid", pad)
        q = conv(torch.cat([round_bf16(r * h), xr], 1), "conv_q", i, "Tanh", pad)
        h = (1 - z) * h + z * q
    return h


def emulated(cxt_channels):
    """``conv_gru_bf16`` with ``conv_gru``'s signature, for ``monkeypatch.setattr(orc, "conv_gru", …)``."""
    def conv_gru(sd, h, x, net_type="SeqConv", prefix="gru"):
        return conv_gru_bf16(sd, h, x, cxt_channels, net_type, prefix)
    return conv_gru


# -------------------------------------------------------------------------------- decoder yardstick
# the tolerances tests/test_gpu_decoder.py grants the fp32 path: mean EPE per sample, |ΔR|, |Δt|
# (atol + rtol·|t|) and the last mask
EPE_TOL, R_ATOL, T_ATOL, T_RTOL, MASK_ATOL = 1e-3, 1e-5, 1e-3, 1e-6, 1e-4
FAMILIES = ("epe_pose", "epe_pred", "dR", "dt", "dmask")


def distances(a, b):
    """Per output family, the distance of decoder outputs ``a`` from ``b`` (the 7 lists of
    SCFlowDecoder.forward): max over samples of the mean EPE of the last pose flow and of the last
    predicted flow, max |ΔR| and max |Δt| over every iteration, max |Δmask| of the last mask."""
    return dict(epe_pose=float(orc.cal_epe_mean(b[0][-1], a[0][-1]).max()),
                epe_pred=float(orc.cal_epe_mean(b[1][-1], a[1][-1]).max()),
                dR=float((torch.stack(a[2]) - torch.stack(b[2])).abs().max()),
                dt=float((torch.stack(a[3]) - torch.stack(b[3])).abs().max()),
                dmask=float((a[4][-1] - b[4][-1]).abs().max()))


def granted(ref):
    """The fp32 path's tolerance per family (``ref``: the fp32 oracle's outputs)."""
    return dict(epe_pose=EPE_TOL, epe_pred=EPE_TOL, dR=R_ATOL,
                dt=T_ATOL + T_RTOL * float(torch.stack(ref[3]).abs().max()), dmask=MASK_ATOL)


@lru_cache(maxsize=None)
def oracle_pair(B, S, seed, iters, w_seed, cxt_channels, feat_size=None):
    """(inputs, decoder, fp32 oracle outputs, emulated-bf16 oracle outputs) for one synthetic
    SCFlowDecoder case, computed once and shared; nothing in it may be modified."""
    from tests.helpers import decoder_inputs
    from tests.test_gpu_decoder import build_decoder
    inp = decoder_inputs(B, S, seed)
    dec = build_decoder(iters, feat_size=feat_size, seed=w_seed)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = orc.decoder_forward(sd, **inp, iters=iters)
    plain = orc.conv_gru
    orc.conv_gru = emulated(cxt_channels)
    try:
        emu = orc.decoder_forward(sd, **inp, iters=iters)
    finally:
        orc.conv_gru = plain
    return inp, dec, ref, emu
