"""GPU: the one weight-packing kernel of the bf16 direct convs (bf16_pack_kernel, conv_bf16_core.h)
against a Python restatement of its layout, bit for bit.

Packed weights are [nb32][k-step][tap][lane][8 bf16], two bf16 per packed float (element 2i in the
low half): lane = li + 32·hh holds output channel 32·nb32 + li, input channels 16·k-step + 8·hh +
0..7; tap = kw·ky + kx; source 1's channels follow source 0's; output channels past cout are 0 up
to the format's padding (64 for 1×5 / 5×1, a 32-channel block for 3×3).  The shapes are the
smallest at which the tap count (5 / 9), the source split (two sources of one stage each: four
k-steps) and the cout padding (a whole zero block; a partly zero block) can each go wrong.
"""
import pytest
import torch

from tests.gru_bf16_restatement import round_bf16

pytestmark = pytest.mark.gpu


def restated(weight, cout_pad):
    """The packed buffer of an OIHW fp32 weight as int32, output channels padded to cout_pad."""
    cout, cin, kh, kw = weight.shape
    taps, nb, nks = kh * kw, cout_pad // 32, cin // 16
    w = torch.zeros(cout_pad, cin, taps)
    w[:cout] = round_bf16(weight).reshape(cout, cin, taps)
    bits = (w.view(torch.int32).to(torch.int64) >> 16) & 0xFFFF
    # [nb, li, ks, hh, e2, pair, tap] → [nb, ks, tap, hh, li, e2, pair]
    bits = bits.view(nb, 32, nks, 2, 4, 2, taps).permute(0, 2, 6, 3, 1, 4, 5)
    u = bits[..., 0] | (bits[..., 1] << 16)
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).reshape(-1)


def packed(weight, c0, c1, fmt):
    from scflow_amd import ops
    out = ops.pack_conv_weight(weight.cuda(), c0, c1, 32, 1, fmt)
    torch.cuda.synchronize()
    return out.cpu().view(torch.int32)


@pytest.mark.parametrize("k", [(1, 5), (5, 1)])
def test_sep_packing_is_the_restated_layout(k):
    from scflow_amd import _lib
    wt = torch.randn(32, 64, *k, generator=torch.Generator().manual_seed(5 + k[0]))
    got = packed(wt, 32, 32, _lib.CONV_BF16)
    assert got.numel() == 64 * 64 * 5 // 2
    assert torch.equal(got, restated(wt, 64))
    assert got[: got.numel() // 2].ne(0).any() and not got[got.numel() // 2:].any()  # the second 32-block


def test_3x3_packing_is_the_restated_layout_in_both_formats():
    from scflow_amd import _lib
    wt = torch.randn(40, 32, 3, 3, generator=torch.Generator().manual_seed(9))
    got = packed(wt, 32, 0, _lib.CONV_BF16_3X3)
    assert got.numel() == 64 * 32 * 9 // 2
    assert torch.equal(got, restated(wt, 64))
    # [nb, ks, tap, hh, li, e2]: rows 40..63 are lanes li ≥ 8 of the second block
    assert not got.view(2, 2, 9, 2, 32, 4)[1, :, :, :, 8:].any()
    assert torch.equal(packed(wt, 32, 0, _lib.CONV_BF16_3X3N), got)
