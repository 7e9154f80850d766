"""Test-side helper (not a test): plain fp64 torch restatement of the pose head's launches, one
function per launch, written from the contract in ``include/scflow_hip.h`` ("a7:
MultiClassPoseHead", ``scflow_enc_conv``'s ``ksplit`` / ``src1`` / ``in_scale`` fields) and not from
the kernels.  No project imports.  ``tests/test_posehead_host.py`` pins the composition of these
functions to ``oracle.scflow_oracle.pose_head``; ``tests/test_gpu_posehead_ops.py`` compares every
launch with them.

Activations are NCHW here (the launches take channels-last slices; the tests transpose), every
result is fp64.
"""
import torch
import torch.nn.functional as F

CHUNK = 16  # channels per K chunk of the gather conv / per K stage of the MFMA conv


def split_bounds(total, parts):
    """The K-split contract shared by the three split launches: slice z of ``parts`` covers the
    units [⌊total·z/parts⌋, ⌊total·(z+1)/parts⌋) — [(lo, hi)] per slice."""
    return [(total * z // parts, total * (z + 1) // parts) for z in range(parts)]


def norm_on_load(x, scale=None, shift=None):
    """relu(x·scale[n, c] + shift[n, c]) of an NCHW tensor (x itself without scale / shift)."""
    x = x.double()
    if scale is None:
        return x
    return torch.relu(x * scale.double()[:, :, None, None] + shift.double()[:, :, None, None])


def conv(x_nchw, w, bias, stride, pad, scale=None, shift=None):
    """The previous GroupNorm + ReLU on load (if given), THEN zero padding, then the conv."""
    x = F.pad(norm_on_load(x_nchw, scale, shift), (pad, pad, pad, pad))
    return F.conv2d(x, w.double(), None if bias is None else bias.double(), stride=stride)


def conv_slab(x_nchw, w, stride, pad, scale, shift, ch_lo, ch_hi):
    """``conv`` (no bias) restricted to the input channels [ch_lo, ch_hi): one K slab of the MFMA
    conv, whose K stages are 16-channel blocks of the concatenated input."""
    sl = slice(ch_lo, ch_hi)
    return conv(x_nchw[:, sl], w[:, sl], None, stride, pad,
                None if scale is None else scale[:, sl], None if shift is None else shift[:, sl])


def chunk_count(cin, kh, kw):
    """K chunks of the gather conv: K is ordered (tap, 16-channel chunk of cin rounded up to 16)."""
    return kh * kw * (-(-cin // CHUNK))


def conv_slab_chunks(x_nchw, w, stride, pad, scale, shift, lo, hi):
    """``conv`` (no bias) restricted to the K chunks [lo, hi) of the gather conv's K order: chunk
    index = tap·⌈cin/16⌉ + (channel // 16), the channels zero-padded to a multiple of 16.  A slab
    whose bounds are no multiple of ⌈cin/16⌉ is cut inside a tap."""
    n, cin = x_nchw.shape[:2]
    cout, _, kh, kw = w.shape
    taps, cch = kh * kw, -(-cin // CHUNK)
    x = F.pad(norm_on_load(x_nchw, scale, shift), (pad, pad, pad, pad))
    oh = (x.shape[2] - kh) // stride + 1
    ow = (x.shape[3] - kw) // stride + 1
    cols = F.unfold(x, (kh, kw), stride=stride).view(n, cin, taps, oh * ow)  # K as (c, tap)
    cols = F.pad(cols, (0, 0, 0, 0, 0, cch * CHUNK - cin))                  # channels → cinp
    cols = cols.permute(0, 2, 1, 3).reshape(n, taps * cch, CHUNK, oh * ow)  # K as (tap, chunk, 16)
    wk = F.pad(w.double().view(cout, cin, taps), (0, 0, 0, cch * CHUNK - cin))
    wk = wk.permute(0, 2, 1).reshape(cout, taps * cch, CHUNK)
    out = torch.einsum("nkcl,okc->nol", cols[:, lo:hi], wk[:, lo:hi])
    return out.view(n, cout, oh, ow)


def chunk_real_k(cin, kh, kw, lo, hi):
    """Terms of the chunks [lo, hi) that are not channel padding (the length of the slab's sum)."""
    cch = -(-cin // CHUNK)
    return sum(min(CHUNK, cin - (kc % cch) * CHUNK) for kc in range(lo, hi))


def gn_affine(y, groups, gamma, beta, eps):
    """GroupNorm(groups) of y [n, c, ...] as a per-(sample, channel) affine: (scale, shift) with
    scale = γ·rstd and shift = β − mean·scale, biased variance (like F.group_norm)."""
    y = y.double()
    n, c = y.shape[:2]
    g = y.reshape(n, groups, -1)
    mean = g.mean(2)
    var = ((g - mean[:, :, None]) ** 2).mean(2)
    rstd = 1.0 / torch.sqrt(var + eps)
    cpg = c // groups
    scale = gamma.double()[None, :] * rstd.repeat_interleave(cpg, 1)
    shift = beta.double()[None, :] - mean.repeat_interleave(cpg, 1) * scale
    return scale, shift


def fc(x, W, bias, relu):
    y = x.double() @ W.double().T
    if bias is not None:
        y = y + bias.double()
    return torch.relu(y) if relu else y


def fc_from_conv(y_nhwc, scale, shift, W_nchw_order, bias, relu):
    """FC on a raw conv output y [m, hw, c] (channels-last): relu(y·scale + shift), flattened in
    NCHW order (column = c·hw + p, nn.Flatten), then the linear layer with the reference's
    weight."""
    a = torch.relu(y_nhwc.double() * scale.double()[:, None, :] + shift.double()[:, None, :])
    return fc(a.permute(0, 2, 1).reshape(a.shape[0], -1), W_nchw_order, bias, relu)


def fc_permute(W, c, hw):
    """W's NCHW-flatten columns (c·hw + p) reordered to channels-last (p·c + c)."""
    return W.view(W.shape[0], c, hw).permute(0, 2, 1).reshape(W.shape[0], hw * c)


def from_partials(parts, xbias):
    """The split producer's output as its consumer reads it: relu(Σ_z parts[z] + xbias)."""
    return torch.relu(parts.double().sum(0) + xbias.double())


def fc_from_partials(parts, xbias, W, bias, relu):
    return fc(from_partials(parts, xbias), W, bias, relu)


def heads(x, Wr, br, Wt, bt, label, rch):
    """(Δrot [m, rch], Δt [m, 3]) from label[0]'s rows of both heads for EVERY sample (the
    reference's index_select(label)[:, 0] quirk)."""
    cls = int(label[0])
    x = x.double()
    r = x @ Wr.double()[cls * rch:(cls + 1) * rch].T + br.double()[cls * rch:(cls + 1) * rch]
    t = x @ Wt.double()[cls * 3:(cls + 1) * 3].T + bt.double()[cls * 3:(cls + 1) * 3]
    return r, t
