"""Tensor-level wrappers over the C ABI (include/scflow_hip.h).

Each wrapper validates devices/dtypes/contiguity, passes raw device pointers and the current
HIP stream of the tensor's device, and raises ``ScflowError`` on any non-zero status.  Inputs
must live on a ROCm device: there is deliberately no CPU path here.

Channels-last activations are described by ``Chan`` = (buffer, first channel, channel count):
the buffer is a contiguous ``[..., C_total]`` tensor, so a ``Chan`` is a channel slice of an
NHWC image with pixel stride ``C_total`` — how the decoder keeps cat[h, cxt, motion, flow] in
one buffer without ever materialising a concatenation.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ScflowError, check

Tensor = torch.Tensor


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: Tensor) -> int:
    """The current HIP stream of t's device as a raw handle (the C entry points take it)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


class BoundCall:
    """A recorded C-ABI launch: a function, its argument tuple (device pointers of persistent
    buffers, sizes, ``byref`` of an argument struct), a device index and a name; the stream is
    taken at call time.  The one way to replay a launch: see ``binding``.  It keeps alive what
    its argument tuple refers to — a struct, and through it the tensors the struct's builder
    attached (``conv2d_args``, ``_pose_step_call``) — and nothing else."""
    __slots__ = ("fn", "args", "dev", "name")

    def __init__(self, fn, args, dev: int, name: str) -> None:
        self.fn, self.args, self.dev, self.name = fn, args, dev, name

    def __call__(self) -> None:
        rc = self.fn(*self.args, raw_stream(self.dev))
        if rc:
            check(rc, self.name)


_BINDING: Optional[list] = None
_BINDING_RUN = True


class binding:
    """``with ops.binding(calls):`` — the wrappers below record their launch as a ``BoundCall``
    into ``calls`` and ALSO run it (so the first pass computes; later passes replay ``calls``,
    costing one ctypes call per launch instead of the wrapper's Python).  ``run=False`` only
    records (the launches are replayed later; their buffers must outlive the replay)."""

    def __init__(self, calls: list, run: bool = True) -> None:
        self.calls, self.run = calls, run

    def __enter__(self):
        global _BINDING, _BINDING_RUN
        self._prev, _BINDING = _BINDING, self.calls
        self._prev_run, _BINDING_RUN = _BINDING_RUN, self.run
        return self.calls

    def __exit__(self, *exc):
        global _BINDING, _BINDING_RUN
        _BINDING, _BINDING_RUN = self._prev, self._prev_run


def host_call(fn) -> None:
    """Run a host-side callable (a kernel-timer hook) in launch order: inside ``binding`` it is
    recorded with the launches (and replayed with them), else it just runs."""
    if _BINDING is not None:
        _BINDING.append(fn)
        if not _BINDING_RUN:
            return
    fn()


def _launch(name: str, dev_tensor: Tensor, *args) -> None:
    fn = getattr(_lib.load(), name)
    if _BINDING is not None:
        bc = BoundCall(fn, args, dev_tensor.device.index, name)
        _BINDING.append(bc)
        if _BINDING_RUN:
            bc()
        return
    check(fn(*args, _stream(dev_tensor)), name)


def raw_stream(device_index: int) -> int:
    """Current HIP stream of a device by index (no Stream object; for per-launch hot paths)."""
    if _raw_stream is not None:
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def _require(t: Tensor, name: str, dtype=torch.float32, contiguous=True) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.device.type != "cuda":
        raise ScflowError(f"{name} is on {t.device}: the SCFlow HIP path only runs on a ROCm GPU "
                          "(no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _require_rows(t: Tensor, name: str) -> None:
    """``t`` [..., c] is a channel slice of a channels-last buffer: unit channel stride and one
    pixel stride (``t.stride(-2)``, a multiple of 4) over all leading dimensions."""
    _require(t, name, contiguous=False)
    ok = t.stride(-1) == 1 and t.stride(-2) >= t.shape[-1] and t.stride(-2) % 4 == 0
    for i in range(t.dim() - 3, -1, -1):
        ok = ok and (t.shape[i] == 1 or t.stride(i) == t.stride(i + 1) * t.shape[i + 1])
    if not ok:
        raise ValueError(f"{name} must be channels-last rows with one pixel stride, got strides "
                         f"{tuple(t.stride())} for shape {tuple(t.shape)}")


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


@dataclass
class Chan:
    """A channel slice [off, off+c) of a contiguous channels-last buffer ``buf[..., C_total]``."""
    buf: Tensor
    off: int
    c: int

    @property
    def stride(self) -> int:
        return self.buf.shape[-1]

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + 4 * self.off

    @staticmethod
    def whole(buf: Tensor) -> "Chan":
        return Chan(buf, 0, buf.shape[-1])


# ------------------------------------------------------------------------------- a1 pyramid
def pyramid_level_shapes(h: int, w: int, num_levels: int) -> List[Tuple[int, int]]:
    return [(h >> l, w >> l) for l in range(num_levels)]


def corr_pyramid(feat1: Tensor, feat2: Tensor, num_levels: int = 4) -> Tuple[Tensor, List[Tensor]]:
    """Returns (one flat buffer, list of level views ``[N·H·W,1,H_l,W_l]``) — the reference's
    CorrelationPyramid output (raft_decoder.py:35-58) as views of one allocation."""
    _require(feat1, "feat1")
    _require(feat2, "feat2")
    if feat1.shape != feat2.shape or feat1.dim() != 4:
        raise ValueError(f"feature shapes differ or are not 4-D: {feat1.shape} {feat2.shape}")
    n, c, h, w = feat1.shape
    lib = _lib.load()
    size = lib.scflow_corr_pyramid_size(n, h, w, num_levels)
    if size <= 0:
        raise ScflowError(f"bad pyramid geometry n={n} h={h} w={w} L={num_levels}")
    buf = torch.empty(size, device=feat1.device, dtype=torch.float32)
    check(lib.scflow_corr_pyramid(_p(feat1), _p(feat2), _p(buf), n, c, h, w, num_levels,
                                  _stream(feat1)), "scflow_corr_pyramid")
    return buf, pyramid_views(buf, n, h, w, num_levels)


def tiled_pyramid_ok(h: int, w: int, num_levels: int) -> bool:
    """Whether scflow_corr_pyramid_tiled supports this geometry."""
    g = 4 << (num_levels - 1)
    return 1 <= num_levels <= 4 and h % 8 == 0 and w % 8 == 0 and h % g == 0 and w % g == 0


def tiled_lookup_ok(h: int, w: int, num_levels: int, radius: int, align_corners: bool) -> bool:
    """Whether scflow_corr_lookup_tiled supports this geometry (its LDS kernel: r in 1..4, and
    without align_corners every windowed level at least 2r+1 wide and tall)."""
    if not tiled_pyramid_ok(h, w, num_levels) or not 1 <= radius <= 4:
        return False
    if not align_corners:
        win = 2 * radius + 4
        for l in range(num_levels):
            hl, wl = h >> l, w >> l
            whole = hl + 2 <= win and wl + 2 <= win
            if not whole and (hl < 2 * radius + 1 or wl < 2 * radius + 1):
                return False
    return True


def corr_pyramid_tiled(feat1: Tensor, feat2: Tensor, num_levels: int = 4) -> Tensor:
    """The pyramid in the TILED layout (scflow_corr_pyramid_tiled: every map in 4×4 tiles of 16
    floats, pooling fused into the GEMM epilogue) as one flat buffer — for ``corr_lookup(...,
    tiled=True)``; ``untile_pyramid`` turns it back into the reference's level views."""
    _require(feat1, "feat1")
    _require(feat2, "feat2")
    if feat1.shape != feat2.shape or feat1.dim() != 4:
        raise ValueError(f"feature shapes differ or are not 4-D: {feat1.shape} {feat2.shape}")
    n, c, h, w = feat1.shape
    if not tiled_pyramid_ok(h, w, num_levels):
        raise ScflowError(f"tiled pyramid needs L <= 4 and h, w multiples of 8 and 4*2^(L-1): "
                          f"h={h} w={w} L={num_levels}")
    lib = _lib.load()
    buf = torch.empty(lib.scflow_corr_pyramid_size(n, h, w, num_levels), device=feat1.device,
                      dtype=torch.float32)
    _launch("scflow_corr_pyramid_tiled", feat1, _p(feat1), _p(feat2), _p(buf), n, c, h, w,
            num_levels)
    return buf


def untile_pyramid(buf: Tensor, n: int, h: int, w: int, num_levels: int) -> List[Tensor]:
    """Level views ``[N·H·W, 1, H_l, W_l]`` (row-major copies) of a tiled pyramid buffer."""
    out, off, P = [], 0, h * w
    for hl, wl in pyramid_level_shapes(h, w, num_levels):
        t = buf[off: off + n * P * hl * wl].view(n * P, hl // 4, wl // 4, 4, 4)
        out.append(t.permute(0, 1, 3, 2, 4).reshape(n * P, 1, hl, wl))
        off += n * P * hl * wl
    return out


def pyramid_views(buf: Tensor, n: int, h: int, w: int, num_levels: int) -> List[Tensor]:
    views, off, P = [], 0, h * w
    for hl, wl in pyramid_level_shapes(h, w, num_levels):
        views.append(buf[off: off + n * P * hl * wl].view(n * P, 1, hl, wl))
        off += n * P * hl * wl
    return views


def pyramid_buffer(levels: Sequence[Tensor], n: int, h: int, w: int) -> Tensor:
    """The flat buffer behind ``levels``; copies on device if they are not views of one."""
    L = len(levels)
    base = levels[0]
    if base.device.type == "cuda" and base.dtype == torch.float32:
        st = base.untyped_storage()
        ok = all(lv.is_contiguous() and lv.untyped_storage().data_ptr() == st.data_ptr()
                 for lv in levels)
        if ok:
            sizes = [n * h * w * hl * wl for hl, wl in pyramid_level_shapes(h, w, L)]
            off0 = base.storage_offset()
            offs = [off0 + sum(sizes[:i]) for i in range(L)]
            if all(lv.storage_offset() == o for lv, o in zip(levels, offs)):
                total = sum(sizes)
                return torch.as_strided(base, (total,), (1,), off0)
    for i, lv in enumerate(levels):
        _require(lv, f"pyramid level {i}", contiguous=False)
    return torch.cat([lv.reshape(-1) for lv in levels])


# ------------------------------------------------------------------------------- a2 lookup
def _require_mask(mask: Tensor, m: int, like: Tensor) -> None:
    """An occlusion mask of the masked entries: contiguous float32, one value per pixel."""
    _require(mask, "mask")
    if mask.numel() != m or mask.device != like.device:
        raise ValueError(f"mask must hold {m} values on {like.device}, got {tuple(mask.shape)} on "
                         f"{mask.device}")


def corr_lookup(pyr: Tensor, flow: Tensor, n: int, h: int, w: int, num_levels: int, radius: int,
                out: Optional[Chan] = None, flow_layout: str = "nchw",
                align_corners: bool = True, tiled: bool = False,
                mask: Optional[Tensor] = None) -> Tensor:
    """Window lookup.  ``mask`` ([n·h·w] or [n·h·w, 1], default None): every sample of pixel m
    is multiplied by ``mask[m]`` where it is stored (scflow_corr_lookup_masked, the reference's
    ``mask_corr``); None calls the unmasked exports.  ``out=None`` → NCHW ``[n, L(2r+1)², h, w]`` (the reference's layout,
    corr_lookup.py:135-136); otherwise written channels-last into ``out``.  ``align_corners``:
    grid_sample's (SCFlow's config True; False: bilinear_sample's default, corr_lookup.py:35).
    ``tiled``: ``pyr`` is a ``corr_pyramid_tiled`` buffer."""
    _require(pyr, "pyramid")
    _require(flow, "flow")
    K = num_levels * (2 * radius + 1) ** 2
    lay = _lib.LAYOUT_NCHW if flow_layout == "nchw" else _lib.LAYOUT_NHWC
    if out is None:
        res = torch.empty(n, K, h, w, device=flow.device, dtype=torch.float32)
        ptr, olay, ostride = res.data_ptr(), _lib.LAYOUT_NCHW, K
    else:
        res = out.buf
        ptr, olay, ostride = out.ptr, _lib.LAYOUT_NHWC, out.stride
    if mask is not None:
        _require_mask(mask, n * h * w, flow)
        _launch("scflow_corr_lookup_masked", flow, _p(pyr), _p(flow), lay, _p(mask), ptr, olay,
                ostride, n, h, w, num_levels, radius, int(bool(align_corners)), int(bool(tiled)))
    elif tiled:
        _launch("scflow_corr_lookup_tiled", flow, _p(pyr), _p(flow), lay, ptr, olay, ostride, n, h,
                w, num_levels, radius, int(bool(align_corners)))
    elif align_corners:
        _launch("scflow_corr_lookup", flow, _p(pyr), _p(flow), lay, ptr, olay, ostride, n, h, w,
                num_levels, radius)
    else:
        _launch("scflow_corr_lookup_ex", flow, _p(pyr), _p(flow), lay, ptr, olay, ostride, n, h, w,
                num_levels, radius, 0)
    return res


def corr_lookup_conv1x1(pyr: Tensor, flow: Tensor, packed: Tensor, bias: Optional[Tensor], out: Chan,
                        n: int, h: int, w: int, num_levels: int, radius: int, cout: int,
                        act: Optional[str] = "ReLU", align_corners: bool = True,
                        mask: Optional[Tensor] = None) -> None:
    """The tiled lookup and corr_net.0 (1×1, weights packed with ``_lib.CONV_1X1W``) in one launch
    (scflow_corr_lookup_conv1x1): ``out`` ← act(W·lookup + bias); ``flow`` [n·h·w, 2] (NHWC).
    ``mask`` ([n·h·w]): act(W·(mask·lookup) + bias) (scflow_corr_lookup_conv1x1_masked)."""
    _require(pyr, "pyramid")
    _require(flow, "flow", contiguous=False)
    _require(packed, "packed weight")
    if bias is not None:
        _require(bias, "bias")
    if out.c != cout:
        raise ValueError(f"out has {out.c} channels, expected {cout}")
    if mask is not None:
        _require_mask(mask, n * h * w, flow)
        _launch("scflow_corr_lookup_conv1x1_masked", flow, _p(pyr), _p(flow), _p(mask), _p(packed),
                _p(bias), out.ptr, out.stride, n, h, w, num_levels, radius, cout,
                _lib.SCFLOW_ACT[act], int(bool(align_corners)))
        return
    _launch("scflow_corr_lookup_conv1x1", flow, _p(pyr), _p(flow), _p(packed), _p(bias), out.ptr,
            out.stride, n, h, w, num_levels, radius, cout, _lib.SCFLOW_ACT[act], int(bool(align_corners)))


def lookup_conv1x1_ok(h: int, w: int, num_levels: int, radius: int, cin: int, cout: int) -> bool:
    """Whether scflow_corr_lookup_conv1x1 supports this geometry."""
    return (num_levels == 4 and radius == 4 and h % 32 == 0 and w % 32 == 0 and cout <= 256 and
            cin == num_levels * (2 * radius + 1) ** 2)


# ------------------------------------------------------------------------------- convolutions
def pack_conv_weight(weight: Tensor, c0: int, c1: int, w: int, stride: int = 1, bk: int = 16) -> Tensor:
    """Pack an nn.Conv2d weight ``[cout, c0+c1, kh, kw]`` for scflow_conv2d (packing format bk:
    K-stage depth 8/16 of the direct conv, or ``_lib.CONV_WINO`` for the Winograd kernel)."""
    _require(weight, "conv weight", contiguous=False)
    weight = weight.detach().contiguous()
    cout, cin, kh, kw = weight.shape
    if cin != c0 + c1:
        raise ValueError(f"weight has {cin} input channels, expected {c0}+{c1}")
    lib = _lib.load()
    size = lib.scflow_conv_packed_size_bk(cout, c0, c1, kh, kw, stride, w, bk)
    if size < 0:
        raise ScflowError(f"no conv kernel for cout={cout} cin={c0}+{c1} k={kh}x{kw} w={w}")
    packed = torch.empty(size, device=weight.device, dtype=torch.float32)
    check(lib.scflow_conv_pack_weights(_p(weight), _p(packed), cout, c0, c1, kh, kw, stride, w, bk,
                                       _stream(weight)), "scflow_conv_pack_weights")
    return packed


def conv_pick_bk(n: int, h: int, w: int, c0: int, c1: int, cout: int, kh: int, kw: int, ph: int,
                 pw: int, stride: int = 1) -> int:
    """The library's preferred packing format for this launch shape (host-only query): the
    direct conv's K-stage depth (8 or 16), ``_lib.CONV_WINO`` or ``_lib.CONV_1X1W``."""
    a = _lib.ConvArgs()
    a.c0, a.c1, a.n, a.h, a.w = c0, c1, n, h, w
    a.cout, a.kh, a.kw, a.ph, a.pw, a.stride = cout, kh, kw, ph, pw, stride
    bk = _lib.load().scflow_conv_pick_bk(ctypes.byref(a))
    if bk not in (8, 16, _lib.CONV_WINO, _lib.CONV_1X1W, _lib.CONV_WINO4):
        check(bk if bk < 0 else -2, "scflow_conv_pick_bk")
    return bk


def conv2d(src0: Chan, packed: Tensor, bias: Optional[Tensor], n: int, h: int, w: int, cout: int,
           kh: int, kw: int, ph: int, pw: int, act: Optional[str] = None, out: Optional[Chan] = None,
           src1: Optional[Chan] = None, epilogue: int = _lib.EPI_PLAIN, gate: Optional[Chan] = None,
           rh: Optional[Chan] = None, hid: Optional[Chan] = None, stride: int = 1,
           bias_map: Optional[Chan] = None, bk: int = 16, **fused) -> None:
    """One scflow_conv2d launch; ``fused``: in_scale / in_shift / out_scale / out_shift / res
    (Winograd 3×3 and ``_lib.CONV_BF16_3X3N`` only, see conv2d_args)."""
    conv2d_launch(conv2d_args(src0, packed, bias, n, h, w, cout, kh, kw, ph, pw, act, out, src1,
                              epilogue, gate, rh, hid, stride, bias_map, bk, **fused), src0.buf)


def conv2d_launch(args, dev_tensor: Tensor) -> None:
    """scflow_conv2d on an argument struct from ``conv2d_args`` / ``ConvRunner.args``."""
    _launch("scflow_conv2d", dev_tensor, ctypes.byref(args))


def conv2d_pair(args_a, args_b, dev_tensor: Tensor) -> None:
    """scflow_conv2d_pair: two independent convs (argument structs from ``ConvRunner.args``; the
    runners keep their packed weights) as one grouped launch where a paired kernel covers them,
    else two launches in order — bit-identical to the separate launches."""
    _launch("scflow_conv2d_pair", dev_tensor, ctypes.byref(args_a), ctypes.byref(args_b))


def conv_plan_kind(args_a, args_b=None) -> int:
    """scflow_conv_plan_kind (host-only): the kernel family scflow_conv2d launches for ``args_a``
    (``_lib.PLAN_*``), or with ``args_b`` the grouped kernel scflow_conv2d_pair launches for the
    two (``_lib.PAIR_*``, 0: two launches); raises what the launch would refuse with."""
    kind = ctypes.c_int(0)
    check(_lib.load().scflow_conv_plan_kind(ctypes.byref(args_a),
                                            ctypes.byref(args_b) if args_b is not None else None,
                                            ctypes.byref(kind)), "scflow_conv_plan_kind")
    return kind.value


def xhead_pred_pack(flow_w: Tensor, mask_w: Tensor) -> Tensor:
    """scflow_xhead_pred's predictor weights: flow predictor [2, cf, 3, 3] and mask predictor
    [1, cm, 1, 1] → [cf + cm, 20] (row c < cf: W[o][c][ty][tx] at column (3·ty + tx)·2 + o; row
    cf + c: the mask weight at column 0)."""
    cf, cm = flow_w.shape[1], mask_w.shape[1]
    pw = torch.zeros(cf + cm, 20, device=flow_w.device, dtype=torch.float32)
    pw[:cf, :18] = flow_w.detach().float().permute(1, 2, 3, 0).reshape(cf, 18)
    pw[cf:, 0] = mask_w.detach().float().reshape(cm)
    return pw


def xhead_pred_workspace(n: int, h: int, w: int, flow_channels: int, hidden_channels: int,
                         device) -> Tensor:
    """The partial-sum workspace of scflow_xhead_pred (float32, 16-byte aligned)."""
    nb = int(_lib.load().scflow_xhead_pred_workspace_bytes(n, h, w, flow_channels, hidden_channels))
    if nb < 0:
        check(nb, "scflow_xhead_pred_workspace_bytes")
    return torch.empty(max(nb // 4, 1), device=device)


def xhead_pred(hidden_args, flow_channels: int, pred_w: Tensor, ws: Tensor,
               flow_bias: Optional[Tensor], mask_bias: Optional[Tensor], flow_act, mask_act,
               flow_out: Chan, mask_out: Chan) -> None:
    """scflow_xhead_pred: the XHeads' hidden conv (argument struct from ``ConvRunner.args``, the
    runner keeps its packed weights) with both predictors contracted in its epilogue, then the
    block / tap sum → flow_out (2 channels), mask_out (1 channel)."""
    _require(pred_w, "pred_w")
    _launch("scflow_xhead_pred", ws, ctypes.byref(hidden_args), flow_channels, _p(pred_w), _p(ws),
            ws.numel() * 4, _p(flow_bias), _p(mask_bias), _lib.SCFLOW_ACT[flow_act], _lib.SCFLOW_ACT[mask_act],
            _p(flow_out.buf) + 4 * flow_out.off, flow_out.buf.shape[1],
            _p(mask_out.buf) + 4 * mask_out.off, mask_out.buf.shape[1])


class SyncEvent:
    """A device-scope cross-stream event (scflow_sync_event_*): ``record(stream)`` then
    ``wait(stream)`` orders the second stream after the first without the system-scope cache
    writeback of a default HIP event.  ``timing=True``: a timing event (``elapsed_ms``)."""

    def __init__(self, timing: bool = False) -> None:
        lib = _lib.load()
        h = ctypes.c_void_p()
        if timing:
            check(lib.scflow_timing_event_create(ctypes.byref(h)), "scflow_timing_event_create")
        else:
            check(lib.scflow_sync_event_create(ctypes.byref(h)), "scflow_sync_event_create")
        self._h, self._lib = h, lib

    def elapsed_ms(self, end: "SyncEvent") -> float:
        """Milliseconds from this (timing) event to ``end`` (waits for ``end``)."""
        ms = ctypes.c_float()
        check(self._lib.scflow_event_elapsed_ms(self._h, end._h, ctypes.byref(ms)),
              "scflow_event_elapsed_ms")
        return float(ms.value)

    def record(self, stream: int) -> None:
        rc = self._lib.scflow_sync_event_record(self._h, stream)
        if rc:
            check(rc, "scflow_sync_event_record")

    def wait(self, stream: int) -> None:
        rc = self._lib.scflow_stream_wait_event(stream, self._h)
        if rc:
            check(rc, "scflow_stream_wait_event")

    def __del__(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.scflow_sync_event_destroy(h)
            except Exception:
                pass


def conv2d_args(src0: Chan, packed: Tensor, bias: Optional[Tensor], n: int, h: int, w: int,
                cout: int, kh: int, kw: int, ph: int, pw: int, act: Optional[str] = None,
                out: Optional[Chan] = None, src1: Optional[Chan] = None,
                epilogue: int = _lib.EPI_PLAIN, gate: Optional[Chan] = None,
                rh: Optional[Chan] = None, hid: Optional[Chan] = None, stride: int = 1,
                bias_map: Optional[Chan] = None, bk: int = 16, in_scale: Optional[Tensor] = None,
                in_shift: Optional[Tensor] = None, out_scale: Optional[Tensor] = None,
                out_shift: Optional[Tensor] = None, res: Optional[Chan] = None) -> "_lib.ConvArgs":
    """The validated scflow_conv_args of one launch (see conv2d).  in_/out_scale/shift and res
    (Winograd 3×3 and the bf16 direct 3×3 conv's encoder form, ``_lib.CONV_BF16_3X3N``, only):
    relu(x·in_scale + in_shift) on load, (conv + b)·out_scale + out_shift, + res before the
    activation.  The struct holds the packed weights and the bias it points at (``_keep``, and
    the workspace in ``_ws``), so whoever holds the struct — a recorded call, ``conv2d_pair``,
    ``xhead_pred`` — keeps them alive."""
    for nm, ch in (("src0", src0), ("src1", src1), ("out", out), ("gate", gate), ("rh", rh),
                   ("hid", hid), ("bias_map", bias_map)):
        if ch is not None:
            _require(ch.buf, nm)
    _require(packed, "packed weight")
    if bias is not None:
        _require(bias, "bias")
    a = _lib.ConvArgs()
    a.src0, a.c0, a.s0 = src0.ptr, src0.c, src0.stride
    if src1 is not None:
        a.src1, a.c1, a.s1 = src1.ptr, src1.c, src1.stride
    a.weight = packed.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a._keep = (packed, bias)
    if out is not None:
        a.out, a.so = out.ptr, out.stride
    a.n, a.h, a.w = n, h, w
    a.cout, a.kh, a.kw, a.ph, a.pw, a.stride = cout, kh, kw, ph, pw, stride
    a.act = _lib.SCFLOW_ACT[act]
    a.epilogue = epilogue
    if gate is not None:
        a.gate, a.sg = gate.ptr, gate.stride
    if rh is not None:
        a.rh, a.srh = rh.ptr, rh.stride
    if hid is not None:
        a.hid, a.sh = hid.ptr, hid.stride
    if bias_map is not None:
        a.bias_map, a.sbm = bias_map.ptr, bias_map.stride
    a.bk = bk
    for nm, t in (("in_scale", in_scale), ("in_shift", in_shift), ("out_scale", out_scale),
                  ("out_shift", out_shift)):
        if t is not None:
            _require(t, nm)
            setattr(a, nm, t.data_ptr())
    if res is not None:
        _require(res.buf, "res")
        a.res, a.sres = res.ptr, res.stride
    if bk == _lib.CONV_WINO4:
        # the transformed-input workspace, private to this launch (a bound launch keeps it with
        # its arguments; an eager one returns it to the stream-ordered caching allocator)
        nb = int(_lib.load().scflow_conv_workspace_bytes(ctypes.byref(a)))
        check(nb if nb < 0 else 0, "scflow_conv_workspace_bytes")
        ws = torch.empty(max(nb // 4, 1), device=src0.buf.device)
        a.ws, a.ws_bytes = ws.data_ptr(), nb
        a._ws = ws
    return a


# ------------------------------------------------------------------------------- pose
def lift_points(depth: Tensor, K: Tensor, R: Tensor, t: Tensor) -> Tensor:
    """[N,H,W,4] float32: object-frame point + validity (pose.py:26-64, dense)."""
    for nm, x in (("depth", depth), ("K", K), ("R", R), ("t", t)):
        _require(x, nm)
    n, h, w = depth.shape
    pts = torch.empty(n, h, w, 4, device=depth.device, dtype=torch.float32)
    _launch("scflow_lift_points", depth,_p(depth), _p(K), _p(R), _p(t), _p(pts), n, h, w)
    return pts


POSE_QUAT_XYZW = 16  # SCFLOW_POSE_QUAT_XYZW


def pose_mode(drot: Tensor, depth_transform: str) -> int:
    """The C-ABI pose-update mode word: depth transform bit | quaternion flag (drot [n, 4])."""
    if drot.dim() != 2 or drot.shape[1] not in (4, 6):
        raise ValueError(f"delta rotation must be [n, 6] (ortho6d) or [n, 4] (quaternion x, y, z, w), "
                         f"got {tuple(drot.shape)}")
    return (0 if depth_transform == "exp" else 1) | (POSE_QUAT_XYZW if drot.shape[1] == 4 else 0)


def pose_update(drot: Tensor, dt: Tensor, R: Tensor, t: Tensor, weight: float = 10.0,
                depth_transform: str = "exp") -> Tuple[Tensor, Tensor]:
    """get_pose_from_delta_pose (pose.py:124-149): drot ortho6d [n, 6] or quaternion [n, 4]."""
    for nm, x in (("drot", drot), ("dt", dt), ("R", R), ("t", t)):
        _require(x, nm)
    mode = pose_mode(drot, depth_transform)
    n = drot.shape[0]
    Ro, to = torch.empty_like(R), torch.empty_like(t)
    _launch("scflow_pose_update", drot, _p(drot), _p(dt), _p(R), _p(t), _p(Ro), _p(to), n,
            float(weight), mode)
    return Ro, to


def pose_flow(R: Tensor, t: Tensor, K: Tensor, points: Tensor, invalid_num: float,
              out: Optional[Tensor] = None) -> Tensor:
    for nm, x in (("R", R), ("t", t), ("K", K), ("points", points)):
        _require(x, nm)
    n, h, w, _ = points.shape
    flow = out if out is not None else torch.empty(n, 2, h, w, device=R.device, dtype=torch.float32)
    _launch("scflow_pose_flow", R,_p(R), _p(t), _p(K), _p(points), _p(flow), n, h, w,
                                       float(invalid_num))
    return flow


def pose_update_flow(drot: Tensor, dt: Tensor, R: Tensor, t: Tensor, K: Tensor, points: Tensor,
                     R_out: Tensor, t_out: Tensor, flow_out: Tensor, invalid_num: float,
                     weight: float = 10.0, depth_transform: str = "exp") -> None:
    for nm, x in (("drot", drot), ("dt", dt), ("R", R), ("t", t), ("K", K), ("points", points),
                  ("R_out", R_out), ("t_out", t_out), ("flow_out", flow_out)):
        _require(x, nm)
    n, h, w, _ = points.shape
    _launch("scflow_pose_update_flow", drot,
        _p(drot), _p(dt), _p(R), _p(t), _p(K), _p(points), _p(R_out), _p(t_out), _p(flow_out), n, h,
        w, float(weight), pose_mode(drot, depth_transform), float(invalid_num))


def pose_step(drot: Tensor, dt: Tensor, R: Tensor, t: Tensor, K: Tensor, points: Tensor,
              R_out: Tensor, t_out: Tensor, flow_out: Tensor, invalid_num: float,
              lr: Tensor, delta: Optional[Tensor], mask: Optional[Tensor], flow_up: Tensor,
              mask_up: Optional[Tensor], h: int, w: int, up_scale: float,
              lr_next: Optional[Chan] = None, hx_next: Optional[Chan] = None,
              weight: float = 10.0, depth_transform: str = "exp", parts: int = 3,
              heads: Optional[tuple] = None, mask_next: Optional[Tensor] = None,
              lrm_next: Optional[Chan] = None) -> None:
    """One launch: ``pose_update_flow`` + ``flow_upsample(lr, delta, mask → flow_up, mask_up)``
    + (if ``lr_next``) the next iteration's ``flow_downsample`` of the new pose flow into
    ``lr_next`` / ``hx_next``, computed from the pose directly (scflow_pose_step_call).
    ``parts``: 1 = only the full-resolution outputs, 2 = only the ↓8 flow.
    ``heads`` (``MultiClassPoseHead.heads_args``): the pose head's rotation / translation heads
    in the same launch — ``drot`` / ``dt`` are then written, not read.
    ``mask_next`` ([n·h·w], the mask just predicted) / ``lrm_next`` (the reference's
    ``mask_flow``): ``lr_next`` still receives the unmasked ↓8 flow, ``lrm_next`` and
    ``hx_next`` receive ``lr_next · mask_next``."""
    for nm, x in (("drot", drot), ("dt", dt), ("R", R), ("t", t), ("K", K), ("points", points),
                  ("R_out", R_out), ("t_out", t_out), ("flow_out", flow_out), ("lr", lr),
                  ("flow_up", flow_up)):
        _require(x, nm)
    n = points.shape[0]
    if lr_next is not None and lr_next.buf.data_ptr() == lr.data_ptr():
        raise ValueError("pose_step: lr_next must not alias lr")
    mode = pose_mode(drot, depth_transform)
    if heads is not None:
        label, x = heads[9], heads[0]
        if label.dtype != torch.int64 or label.device != x.device:
            raise TypeError("label must be an int64 tensor on the same device")
    if mask_next is not None or lrm_next is not None:
        if lr_next is None:
            raise ValueError("pose_step: mask_next / lrm_next need lr_next")
        if mask_next is not None:
            _require_mask(mask_next, n * h * w, lr)
        if lrm_next is not None and lrm_next.buf.data_ptr() in (lr.data_ptr(),
                                                                lr_next.buf.data_ptr()):
            raise ValueError("pose_step: lrm_next must alias neither lr nor lr_next")
    _pose_step_call(drot=drot, dt=dt, R=R, t=t, K=K, points=points, R_out=R_out, t_out=t_out,
                    flow_out=flow_out, invalid_num=invalid_num, lr=lr, delta=delta, mask=mask,
                    flow_up=flow_up, mask_up=mask_up, h=h, w=w, up_scale=up_scale, lr_next=lr_next,
                    hx_next=hx_next, weight=weight, mode=mode,
                    parts=parts, heads=heads, mask_next=mask_next, lrm_next=lrm_next)


def _pose_step_call(*, R, t, K, points, flow_out, invalid_num, lr, delta, mask, flow_up, mask_up, h,
                    w, up_scale, drot=None, dt=None, R_out=None, t_out=None, lr_next=None,
                    hx_next=None, weight=10.0, mode=0, parts=1, heads=None, mask_next=None,
                    lrm_next=None) -> None:
    """Fill scflow_pose_step_args by field name (unset: NULL / 0) and launch
    scflow_pose_step_call.  ``drot`` None is the given-pose form (R, t are the updated pose).
    The struct holds the tensors it points at (``_keep``): a recorded call keeps them alive."""
    a = _lib.PoseStepArgs()
    keep = [drot, dt, R, t, K, points, R_out, t_out, flow_out, lr, delta, mask, flow_up, mask_up,
            mask_next]
    if heads is not None:
        x, xsplit, xbias, k, Wr, br, rch, Wt, bt, label, num_class = heads
        a.x, a.xsplit, a.xbias, a.k = _p(x), int(xsplit), _p(xbias), int(k)
        a.Wr, a.br, a.rch, a.Wt, a.bt = _p(Wr), _p(br), int(rch), _p(Wt), _p(bt)
        a.label, a.num_class = _p(label), int(num_class)
        keep += [x, xbias, Wr, br, Wt, bt, label]
    a.drot, a.dt, a.R_src, a.t_src, a.K, a.points = _p(drot), _p(dt), _p(R), _p(t), _p(K), _p(points)
    a.R_dst, a.t_dst, a.flow = _p(R_out), _p(t_out), _p(flow_out)
    a.n, a.H, a.W = points.shape[:3]
    a.weight, a.depth_transform, a.invalid_num = float(weight), int(mode), float(invalid_num)
    a.lr, a.delta, a.mask, a.flow_up, a.mask_up = _p(lr), _p(delta), _p(mask), _p(flow_up), _p(mask_up)
    a.h, a.w, a.up_scale, a.down_scale = h, w, float(up_scale), 1.0 / float(up_scale)
    for ch, ptr, stride in ((lr_next, "lr_next", "s_next"), (hx_next, "hx_next", "s_hx"),
                            (lrm_next, "lrm_next", "s_lrm")):
        if ch is not None:
            setattr(a, ptr, ch.ptr)
            setattr(a, stride, ch.stride)
            keep.append(ch.buf)
    a.mask_next, a.parts = _p(mask_next), int(parts)
    a._keep = keep
    _launch("scflow_pose_step_call", R, ctypes.byref(a))


def pose_step_given(R: Tensor, t: Tensor, K: Tensor, points: Tensor, flow_out: Tensor,
                    invalid_num: float, lr: Tensor, delta: Optional[Tensor], mask: Optional[Tensor],
                    flow_up: Tensor, mask_up: Optional[Tensor], h: int, w: int,
                    up_scale: float) -> None:
    """``pose_step``'s full-resolution part (parts = 1) from an already updated pose R, t (the ↓8
    part's R_out / t_out): pose flow, ×8 flow prediction and mask, no pose update (the same
    struct with drot = NULL)."""
    for nm, x in (("R", R), ("t", t), ("K", K), ("points", points), ("flow_out", flow_out),
                  ("lr", lr), ("flow_up", flow_up)):
        _require(x, nm)
    _pose_step_call(R=R, t=t, K=K, points=points, flow_out=flow_out, invalid_num=invalid_num, lr=lr,
                    delta=delta, mask=mask, flow_up=flow_up, mask_up=mask_up, h=h, w=w,
                    up_scale=up_scale)


# ------------------------------------------------------------------------------- RANSAC-PnP
PNP_MAX_HYPS = _lib.PNP_MAX_HYPS


def pnp_workspace_bytes(n: int, h: int, w: int, hyps: int) -> int:
    """Bytes of ``pnp_compact``'s workspace (scflow_pnp_workspace: host only, needs no GPU)."""
    nb = ctypes.c_longlong(0)
    check(_lib.load().scflow_pnp_workspace(n, h, w, hyps, ctypes.byref(nb)), "scflow_pnp_workspace")
    return nb.value


def pnp_compact(points: Tensor, flow: Tensor, valid: Optional[Tensor] = None
                ) -> Tuple[Tensor, Tensor]:
    """points [N, H, W, 4] (``lift_points``), flow [N, 2, H, W], valid [N, H, W] float (non-zero =
    keep) or None → (corr [N, H·W, 5], count [N] int32): the valid pixels' (X, Y, Z, x + flow_x,
    y + flow_y) in ascending pixel order in corr[b, :count[b]]; later rows are unspecified."""
    _require(points, "points")
    _require(flow, "flow")
    n, h, w, _ = points.shape
    if tuple(flow.shape) != (n, 2, h, w):
        raise ValueError(f"flow must be {(n, 2, h, w)}, got {tuple(flow.shape)}")
    if valid is not None:
        _require(valid, "valid")
        if valid.numel() != n * h * w:
            raise ValueError(f"valid must have {n * h * w} elements, got {tuple(valid.shape)}")
    ws = torch.empty(pnp_workspace_bytes(n, h, w, 1), device=points.device, dtype=torch.uint8)
    corr = torch.empty(n, h * w, 5, device=points.device, dtype=torch.float32)
    count = torch.empty(n, device=points.device, dtype=torch.int32)
    _launch("scflow_pnp_compact", points, _p(points), _p(flow), _p(valid), _p(corr), _p(count),
            _p(ws), ws.numel(), n, h, w)
    return corr, count


def _require_pnp(corr: Tensor, count: Tensor) -> Tuple[int, int]:
    _require(corr, "corr")
    _require(count, "count", dtype=torch.int32)
    if corr.dim() != 3 or corr.shape[2] != 5 or count.numel() != corr.shape[0]:
        raise ValueError(f"corr must be [N, H·W, 5] with count [N], got {tuple(corr.shape)} / "
                         f"{tuple(count.shape)}")
    return corr.shape[0], corr.shape[1]


def pnp_hypotheses(corr: Tensor, count: Tensor, K: Tensor, hyps: int = 100, seed: int = 0
                   ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """→ (hyp [N, hyps, 12] = K·[R|t], hyp_pose [N, hyps, 12] = [R|t], hyp_valid [N, hyps] int32,
    samples [N, hyps, 4] int32): P3P in fp64 on counter-hashed 4-row samples (scflow_pnp_hypotheses)."""
    n, hw = _require_pnp(corr, count)
    _require(K, "K")
    dev = corr.device
    hyp = torch.empty(n, hyps, 12, device=dev, dtype=torch.float32)
    pose = torch.empty(n, hyps, 12, device=dev, dtype=torch.float32)
    hv = torch.empty(n, hyps, device=dev, dtype=torch.int32)
    samples = torch.empty(n, hyps, 4, device=dev, dtype=torch.int32)
    _launch("scflow_pnp_hypotheses", corr, _p(corr), _p(count), _p(K), _p(hyp), _p(pose), _p(hv),
            _p(samples), n, hw, int(hyps), int(seed) & 0xFFFFFFFF)
    return hyp, pose, hv, samples


def pnp_score(corr: Tensor, count: Tensor, hyp: Tensor, hyp_valid: Tensor, thr: float = 3.0
              ) -> Tensor:
    """score [N, hyps] int32: rows in front of the camera with reprojection error < thr under each
    hypothesis, 0 for invalid ones (scflow_pnp_score)."""
    n, hw = _require_pnp(corr, count)
    _require(hyp, "hyp")
    _require(hyp_valid, "hyp_valid", dtype=torch.int32)
    hyps = hyp.shape[1]
    if tuple(hyp.shape) != (n, hyps, 12) or tuple(hyp_valid.shape) != (n, hyps):
        raise ValueError(f"hyp / hyp_valid must be [N, hyps, 12] / [N, hyps], got "
                         f"{tuple(hyp.shape)} / {tuple(hyp_valid.shape)}")
    score = torch.empty(n, hyps, device=corr.device, dtype=torch.int32)
    _launch("scflow_pnp_score", corr, _p(corr), _p(count), _p(hyp), _p(hyp_valid), _p(score), n, hw,
            hyps, float(thr))
    return score


def pnp_refine(corr: Tensor, count: Tensor, hyp: Tensor, hyp_pose: Tensor, hyp_valid: Tensor,
               score: Tensor, K: Tensor, R: Tensor, t: Tensor, thr: float = 3.0,
               refine_iters: int = 10, pose64: Optional[Tensor] = None
               ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Winner per sample + Gauss-Newton on its inliers (scflow_pnp_refine) → (R [N, 3, 3],
    t [N, 3], ok [N] int32, inliers [N] int32); the reference pose R, t where ok is 0.  pose64
    [N, 12] float64, when given, receives the pose before its rounding to fp32 (R, then t)."""
    n, hw = _require_pnp(corr, count)
    if pose64 is not None:
        _require(pose64, "pose64", dtype=torch.float64)
        if tuple(pose64.shape) != (n, 12):
            raise ValueError(f"pose64 must be {(n, 12)}, got {tuple(pose64.shape)}")
    for nm, x in (("hyp", hyp), ("hyp_pose", hyp_pose), ("K", K), ("R", R), ("t", t)):
        _require(x, nm)
    _require(hyp_valid, "hyp_valid", dtype=torch.int32)
    _require(score, "score", dtype=torch.int32)
    hyps = hyp.shape[1]
    if tuple(hyp.shape) != (n, hyps, 12) or hyp_pose.shape != hyp.shape or \
            tuple(hyp_valid.shape) != (n, hyps) or tuple(score.shape) != (n, hyps):
        raise ValueError("hyp, hyp_pose [N, hyps, 12] and hyp_valid, score [N, hyps] must agree")
    Ro, to = torch.empty_like(R), torch.empty_like(t)
    ok = torch.empty(n, device=corr.device, dtype=torch.int32)
    inl = torch.empty(n, device=corr.device, dtype=torch.int32)
    _launch("scflow_pnp_refine", corr, _p(corr), _p(count), _p(hyp), _p(hyp_pose), _p(hyp_valid),
            _p(score), _p(K), _p(R), _p(t), _p(Ro), _p(to), _p(ok), _p(inl), _p(pose64), n, hw,
            hyps, float(thr), int(refine_iters))
    return Ro, to, ok, inl


def pnp_ransac(flow: Tensor, depth: Tensor, R: Tensor, t: Tensor, K: Tensor,
               valid: Optional[Tensor] = None, hyps: int = 100, thr: float = 3.0,
               refine_iters: int = 10, seed: int = 0, pose64: Optional[Tensor] = None
               ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Batched RANSAC-PnP: flow [B, 2, H, W], rendered depth [B, H, W], reference
    pose R [B, 3, 3], t [B, 3], intrinsics K [B, 3, 3], valid [B, H, W] (bool or float, non-zero =
    use the pixel) → (R [B, 3, 3], t [B, 3], ok [B] bool, inliers [B] int32).  Lift → compact →
    hypotheses → score → refine on the current stream, no host synchronisation; where ok is False
    the pose is the reference pose bit for bit and inliers is 0.  pose64 [B, 12] float64, when
    given, receives the pose before its rounding to fp32 (``pnp_refine``)."""
    if hyps < 1 or hyps > PNP_MAX_HYPS:
        raise ScflowError(f"pnp_ransac: hyps must be in [1, {PNP_MAX_HYPS}], got {hyps}")
    if valid is not None and valid.dtype != torch.float32:
        valid = valid.to(torch.float32)
    points = lift_points(depth, K, R, t)
    corr, count = pnp_compact(points, flow, None if valid is None else valid.contiguous())
    hyp, pose, hv, _ = pnp_hypotheses(corr, count, K, hyps, seed)
    score = pnp_score(corr, count, hyp, hv, thr)
    Ro, to, ok, inl = pnp_refine(corr, count, hyp, pose, hv, score, K, R, t, thr, refine_iters,
                                 pose64)
    return Ro, to, ok != 0, inl


# ------------------------------------------------------------------------------- patches
PATCH_MAX_CROP = _lib.PATCH_MAX_CROP


def _require_patch(t: Tensor, name: str, dtype, shape: Optional[tuple] = None) -> None:
    """The patch ops' argument check: every refusal (type, device, dtype, contiguity, shape; a
    None in ``shape`` matches any extent) is a ``ScflowError`` raised before device work."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor):
        raise ScflowError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise ScflowError(f"{name} is on {t.device}: the patch kernels only run on a ROCm GPU "
                          "(no CPU fallback)")
    if t.dtype not in dtypes:
        raise ScflowError(f"{name} must be {' or '.join(map(str, dtypes))}, got {t.dtype}")
    if not t.is_contiguous():
        raise ScflowError(f"{name} must be contiguous")
    if shape is not None and (t.dim() != len(shape) or any(
            s is not None and s != d for s, d in zip(shape, t.shape))):
        want = "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
        raise ScflowError(f"{name} must be {want}, got {list(t.shape)}")


def _require_patch_size(size: int) -> None:
    if size < 4 or size > 4096 or size % 4:
        raise ScflowError(f"the patch side must be a multiple of 4 in [4, 4096], got {size}")


def patch_staged(cw: int, channels: int, dtype=torch.uint8, size: int = 256) -> bool:
    """Whether ``extract_patches`` stages the source rows of a crop ``cw`` pixels wide in LDS
    (scflow_patch_staged: host only, follows SCFLOW_PATCH_LDS) or reads its taps directly."""
    rc = _lib.load().scflow_patch_staged(int(cw), int(channels),
                                         _lib.PATCH_U8 if dtype == torch.uint8 else _lib.PATCH_F32,
                                         int(size))
    if rc < 0:
        check(rc, "scflow_patch_staged")
    return rc == 1


def patch_boxes(points: Tensor, counts: Tensor, labels: Tensor, R: Tensor, t: Tensor, ori_k: Tensor,
                ratio: Tensor, height: int, width: int, size: int,
                frame_index: Optional[Tensor] = None, num_frames: int = 0,
                k_per_frame: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Crop geometry of N objects from their projected model points (scflow_patch_boxes; DESIGN.md
    §15): points [C, P, 3] with counts [C] int32, labels [N] int32, R [N, 3, 3], t [N, 3], ori_k
    [N, 3, 3] — or [num_frames, 3, 3] with ``k_per_frame``, indexed by frame_index [N] int32 —
    ratio [N], the frame's height × width and the patch side → (bbox [N, 4] (l, t, r, b), geom
    [N, 8] int32 (x1, y1, x2, y2, nw, nh, left, top), T [N, 3, 3], k [N, 3, 3] = T·ori_k, valid [N]
    uint8).  One launch on the current stream; with frame_index an index outside [0, num_frames)
    makes its object invalid.  N = 0 returns empty tensors without a launch."""
    _require_patch_size(size)
    _require_patch(points, "points", torch.float32, (None, None, 3))
    c, p, _ = points.shape
    _require_patch(counts, "counts", torch.int32, (c,))
    _require_patch(labels, "labels", torch.int32, (None,))
    n = labels.shape[0]
    _require_patch(R, "R", torch.float32, (n, 3, 3))
    _require_patch(t, "t", torch.float32, (n, 3))
    _require_patch(ratio, "ratio", torch.float32, (n,))
    if k_per_frame and frame_index is None:
        raise ScflowError("patch_boxes: ori_k per frame needs frame_index")
    if frame_index is not None:
        _require_patch(frame_index, "frame_index", torch.int32, (n,))
        if num_frames < 1:
            raise ScflowError(f"patch_boxes: frame_index needs num_frames ≥ 1, got {num_frames}")
    _require_patch(ori_k, "ori_k", torch.float32, (num_frames if k_per_frame else n, 3, 3))
    if c < 1 or p < 1 or height < 1 or width < 1:
        raise ScflowError(f"patch_boxes: empty point table {list(points.shape)} or frame "
                          f"{height}×{width}")
    dev = labels.device
    bbox = torch.empty(n, 4, device=dev, dtype=torch.float32)
    geom = torch.empty(n, 8, device=dev, dtype=torch.int32)
    T = torch.empty(n, 3, 3, device=dev, dtype=torch.float32)
    k = torch.empty(n, 3, 3, device=dev, dtype=torch.float32)
    valid = torch.empty(n, device=dev, dtype=torch.uint8)
    if n:
        _launch("scflow_patch_boxes", labels, _p(points), _p(counts), _p(labels), _p(R), _p(t),
                _p(ori_k), _p(frame_index), _p(ratio), _p(bbox), _p(geom), _p(T), _p(k), _p(valid),
                n, c, p, int(bool(k_per_frame)), int(num_frames), int(height), int(width),
                int(size))
    return bbox, geom, T, k, valid


def extract_patches(frames: Tensor, frame_index: Tensor, geom: Tensor, valid: Tensor, size: int,
                    pad: float = 128.0, mean: Optional[Sequence[float]] = None,
                    std: Optional[Sequence[float]] = None, to_rgb: bool = False,
                    quantize: bool = True, nearest: bool = False) -> Tensor:
    """Crop, resize and pad N patches in one launch (scflow_patch_extract): frames
    [F, H, W, 3] uint8 (interleaved) or [F, H, W, 1] uint8 / float32, frame_index [N] int32, geom
    [N, 8] int32 and valid [N] uint8 of ``patch_boxes`` → [N, C, size, size] float32, planar:
    cv2's INTER_LINEAR of the inclusive crop (``nearest``: the nearest source pixel), rounded to
    integer levels with ``quantize``, ``pad`` outside the frame and around the resized crop, then
    (v − mean[c]) / std[c] per output channel, the channel order reversed first with ``to_rgb``.
    An invalid object's patch is ``pad`` everywhere.  Runs on the current stream; N = 0 returns an
    empty tensor without a launch."""
    _require_patch_size(size)
    _require_patch(frames, "frames", (torch.uint8, torch.float32), (None, None, None, None))
    f, h, w, c = frames.shape
    if not (c == 1 or (c == 3 and frames.dtype == torch.uint8)):
        raise ScflowError("frames must be [F, H, W, 3] uint8 or [F, H, W, 1] uint8 / float32, got "
                          f"{list(frames.shape)} {frames.dtype}")
    if f < 1 or h < 1 or w < 1:
        raise ScflowError(f"frames must not be empty, got {list(frames.shape)}")
    _require_patch(frame_index, "frame_index", torch.int32, (None,))
    n = frame_index.shape[0]
    _require_patch(geom, "geom", torch.int32, (n, 8))
    _require_patch(valid, "valid", torch.uint8, (n,))
    stats = []
    for name, v, dflt in (("mean", mean, 0.0), ("std", std, 1.0)):
        v = [dflt] * c if v is None else [float(x) for x in v]
        if len(v) != c:
            raise ScflowError(f"{name} must have {c} entries, got {len(v)}")
        stats.append((ctypes.c_float * c)(*v))
    if any(s == 0.0 for s in stats[1]):
        raise ScflowError("std must not be zero")
    out = torch.empty(n, c, size, size, device=frames.device, dtype=torch.float32)
    if n:
        flags = (_lib.PATCH_TO_RGB if to_rgb else 0) | (_lib.PATCH_QUANTIZE if quantize else 0) | \
            (_lib.PATCH_NEAREST if nearest else 0)
        _launch("scflow_patch_extract", frames, _p(frames), _p(frame_index), _p(geom), _p(valid),
                _p(out), n, f, h, w, c,
                _lib.PATCH_U8 if frames.dtype == torch.uint8 else _lib.PATCH_F32, int(size),
                float(pad), ctypes.cast(stats[0], ctypes.c_void_p),
                ctypes.cast(stats[1], ctypes.c_void_p), flags)
    return out


def _require_counter(seed: int, step: int, object_offset: int) -> None:
    if not (0 <= seed < 2 ** 64 and 0 <= step < 2 ** 56 and 0 <= object_offset < 2 ** 32):
        raise ScflowError(f"seed must be in [0, 2^64), step in [0, 2^56) and object_offset in "
                          f"[0, 2^32), got {seed}, {step}, {object_offset}")


def philox4x32(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """One Philox4x32-10 call as the kernels make it (scflow_philox4x32: host only)."""
    c, k, o = (ctypes.c_uint * 4)(*counter), (ctypes.c_uint * 2)(*key), (ctypes.c_uint * 4)()
    _lib.load().scflow_philox4x32(ctypes.cast(c, ctypes.c_void_p), ctypes.cast(k, ctypes.c_void_p),
                                  ctypes.cast(o, ctypes.c_void_p))
    return tuple(o)


def train_draw(points: Tensor, counts: Tensor, labels: Tensor, diameters: Tensor, R_gt: Tensor,
               t_gt: Tensor, cfg: dict, seed: int, step: int, object_offset: int = 0,
               max_tries: int = 32
               ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Pose jitter, crop ratio and colour parameters of N objects in one launch (scflow_train_draw;
    DESIGN.md §17; the reference's PoseJitter, Crop's size draw and the draws of RandomHSV /
    RandomNoise / RandomSmooth): points [C, P, 3] with counts [C] int32 and diameters [C], labels
    [N] int32, GT poses R_gt [N, 3, 3] / t_gt [N, 3], ``cfg`` a dict with the keys of
    ``_lib.TRAIN_CFG`` plus ``max_kernel_size`` (``patches.TRAIN_AUG`` holds the config's) →
    (R_ref [N, 3, 3], t_ref [N, 3], errors [N, 3] = (add, rot, trans), ok [N] uint8, tries [N]
    int32, ratio [N], aug [N, 8]).  Everything is a function of (seed, step, object_offset + i)
    alone.  Runs on the current stream; N = 0 returns empty tensors without a launch."""
    _require_patch(points, "points", torch.float32, (None, None, 3))
    c, p, _ = points.shape
    _require_patch(counts, "counts", torch.int32, (c,))
    _require_patch(diameters, "diameters", torch.float32, (c,))
    _require_patch(labels, "labels", torch.int32, (None,))
    n = labels.shape[0]
    _require_patch(R_gt, "R_gt", torch.float32, (n, 3, 3))
    _require_patch(t_gt, "t_gt", torch.float32, (n, 3))
    _require_counter(seed, step, object_offset)
    missing = [k for k in _lib.TRAIN_CFG + ("max_kernel_size",) if k not in cfg]
    if missing:
        raise ScflowError(f"train_draw: cfg lacks {missing}")
    mk = int(cfg["max_kernel_size"])
    if not (1 <= mk <= 5 and 0 <= max_tries <= _lib.TRAIN_MAX_TRIES):
        raise ScflowError(f"train_draw: max_kernel_size must be in [1, 5] and max_tries in "
                          f"[0, {_lib.TRAIN_MAX_TRIES}], got {mk}, {max_tries}")
    if c < 1 or p < 1:
        raise ScflowError(f"train_draw: empty point table {list(points.shape)}")
    host = (ctypes.c_float * len(_lib.TRAIN_CFG))(*[float(cfg[k]) for k in _lib.TRAIN_CFG])
    dev = labels.device
    new = lambda *s, dt=torch.float32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
    R, t, err, ratio, aug = new(n, 3, 3), new(n, 3), new(n, 3), new(n), new(n, 8)
    ok, tries = new(n, dt=torch.uint8), new(n, dt=torch.int32)
    if n:
        _launch("scflow_train_draw", labels, _p(points), _p(counts), _p(labels), _p(diameters),
                _p(R_gt), _p(t_gt), ctypes.cast(host, ctypes.c_void_p), _p(R), _p(t), _p(err),
                _p(ok), _p(tries), _p(ratio), _p(aug), n, c, p, int(max_tries), mk, int(seed),
                int(step), int(object_offset))
    return R, t, err, ok, tries, ratio, aug


def _require_aug_extract(frames, frame_index, geom, valid, aug, size, seed, step, object_offset,
                         pad, mean, std):
    """The argument checks ``extract_patches_aug`` and ``extract_patches_aug_bg`` share → (n, f, h,
    w, (mean, std) as host arrays)."""
    _require_patch_size(size)
    _require_patch(frames, "frames", torch.uint8, (None, None, None, 3))
    f, h, w, _ = frames.shape
    if f < 1 or h < 1 or w < 1:
        raise ScflowError(f"frames must not be empty, got {list(frames.shape)}")
    _require_patch(frame_index, "frame_index", torch.int32, (None,))
    n = frame_index.shape[0]
    _require_patch(geom, "geom", torch.int32, (n, 8))
    _require_patch(valid, "valid", torch.uint8, (n,))
    _require_patch(aug, "aug", torch.float32, (n, 8))
    _require_counter(seed, step, object_offset)
    if int(pad) != pad or not 0 <= pad <= 255:
        raise ScflowError(f"pad must be an integer level in [0, 255], got {pad}")
    stats = []
    for name, v, dflt in (("mean", mean, 0.0), ("std", std, 1.0)):
        v = [dflt] * 3 if v is None else [float(x) for x in v]
        if len(v) != 3:
            raise ScflowError(f"{name} must have 3 entries, got {len(v)}")
        stats.append((ctypes.c_float * 3)(*v))
    if any(s == 0.0 for s in stats[1]):
        raise ScflowError("std must not be zero")
    return n, f, h, w, stats


def extract_patches_aug(frames: Tensor, frame_index: Tensor, geom: Tensor, valid: Tensor,
                        aug: Tensor, size: int, seed: int, step: int, object_offset: int = 0,
                        pad: int = 128, mean: Optional[Sequence[float]] = None,
                        std: Optional[Sequence[float]] = None, to_rgb: bool = False,
                        quantize: bool = True, direct: bool = False) -> Tensor:
    """``extract_patches`` for [F, H, W, 3] uint8 BGR frames with the training pipeline's colour
    stages on the crop, before the resize, in the same launch (scflow_train_patch_extract; DESIGN.md
    §17): aug [N, 8] float32 = (a, b, c, sigma, ksize, stage mask, 0, 0) per object, as
    ``train_draw`` returns it or as the caller writes it — HSV gains, the noise's sigma (its
    normals come from (seed, step, object_offset + i, crop pixel)), the box blur's side (1, 3 or
    5) and which stages run (``_lib.AUG_*``).  ``pad`` is an integer level.  A stage mask of 0 gives
    ``extract_patches``' bits.  ``direct`` forces the route that stages nothing in LDS (the same
    bits).  Runs on the current stream; N = 0 returns an empty tensor without a launch."""
    n, f, h, w, stats = _require_aug_extract(frames, frame_index, geom, valid, aug, size, seed, step,
                                             object_offset, pad, mean, std)
    out = torch.empty(n, 3, size, size, device=frames.device, dtype=torch.float32)
    if n:
        flags = (_lib.PATCH_TO_RGB if to_rgb else 0) | (_lib.PATCH_QUANTIZE if quantize else 0) | \
            (_lib.PATCH_AUG_DIRECT if direct else 0)
        _launch("scflow_train_patch_extract", frames, _p(frames), _p(frame_index), _p(geom),
                _p(valid), _p(aug), _p(out), n, f, h, w, int(size), int(pad),
                ctypes.cast(stats[0], ctypes.c_void_p), ctypes.cast(stats[1], ctypes.c_void_p),
                flags, int(seed), int(step), int(object_offset))
    return out


def extract_patches_aug_bg(frames: Tensor, masks: Tensor, frame_index: Tensor, geom: Tensor,
                           valid: Tensor, aug: Tensor, backgrounds: Tensor, size: int, seed: int,
                           step: int, object_offset: int = 0, p: float = 0.3,
                           background_sizes: Optional[Tensor] = None,
                           background_index: Optional[Tensor] = None, pad: int = 128,
                           mean: Optional[Sequence[float]] = None,
                           std: Optional[Sequence[float]] = None, to_rgb: bool = False,
                           quantize: bool = True, direct: bool = False) -> Tuple[Tensor, Tensor]:
    """``extract_patches_aug`` with the reference's RandomBackground between the crop and the
    colour stages, in the same launch (scflow_train_patch_extract_bg): ``masks``
    [F, H, W] uint8 (foreground where != 0), ``backgrounds`` [B, Hb, Wb, 3] uint8 BGR with
    ``background_sizes`` [B, 2] int32 = the used (height, width) of every slot, top-left aligned
    (None: the whole slot).  With probability ``p`` an object takes one slot, drawn uniformly from
    (seed, step, object_offset + i); every crop pixel outside the frame or with a zero mask byte
    then becomes the slot's used region resampled bilinearly to the crop's own size, and the stages
    run on the composite.  ``background_index`` [N] int32 replaces the draw: −1 none, 0 … B−1 that
    slot, anything else none.  Returns (patches [N, 3, size, size], chosen [N] int32: the slot
    applied, −1 for none).

    ``background_sizes`` on the host (a CPU tensor) is checked here, row by row, and copied to the
    pool's device; a device tensor is used as it is, without a synchronisation, and a row that is
    no used size of its slot leaves the objects that draw it without a background (chosen −1).
    Runs on the current stream; N = 0 returns empty tensors without a launch."""
    if not isinstance(backgrounds, torch.Tensor) or backgrounds.dtype != torch.uint8 or \
            backgrounds.dim() != 4 or backgrounds.shape[3] != 3 or 0 in backgrounds.shape:
        got = f"{list(backgrounds.shape)} {backgrounds.dtype}" \
            if isinstance(backgrounds, torch.Tensor) else type(backgrounds).__name__
        raise ScflowError(f"backgrounds must be a non-empty [B, Hb, Wb, 3] uint8 tensor, got {got}")
    b, hb, wb, _ = backgrounds.shape
    sizes = background_sizes
    if sizes is not None:
        if not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int32 or \
                tuple(sizes.shape) != (b, 2):
            raise ScflowError(f"background_sizes must be a [{b}, 2] int32 tensor")
        if sizes.device.type == "cpu":
            bad = ((sizes < 1) | (sizes > torch.tensor([hb, wb], dtype=torch.int32))).any(1)
            if bad.any():
                i = int(bad.nonzero()[0])
                raise ScflowError(f"background_sizes[{i}] = {sizes[i].tolist()} is no used size of a "
                                  f"{hb} × {wb} slot")
    if not 0.0 <= float(p) <= 1.0:  # a NaN fails both comparisons
        raise ScflowError(f"p must be a probability in [0, 1], got {p}")
    n, f, h, w, stats = _require_aug_extract(frames, frame_index, geom, valid, aug, size, seed, step,
                                             object_offset, pad, mean, std)
    _require_patch(masks, "masks", torch.uint8, (f, h, w))
    _require_patch(backgrounds, "backgrounds", torch.uint8)
    if sizes is not None:
        if sizes.device.type == "cpu":
            sizes = sizes.to(backgrounds.device)
        _require_patch(sizes, "background_sizes", torch.int32)
    if background_index is not None:
        _require_patch(background_index, "background_index", torch.int32, (n,))
    out = torch.empty(n, 3, size, size, device=frames.device, dtype=torch.float32)
    chosen = torch.empty(n, device=frames.device, dtype=torch.int32)
    if n:
        flags = (_lib.PATCH_TO_RGB if to_rgb else 0) | (_lib.PATCH_QUANTIZE if quantize else 0) | \
            (_lib.PATCH_AUG_DIRECT if direct else 0)
        _launch("scflow_train_patch_extract_bg", frames, _p(frames), _p(frame_index), _p(geom),
                _p(valid), _p(aug), _p(out), _p(masks), _p(backgrounds), _p(sizes),
                _p(background_index), _p(chosen), n, f, h, w, int(size), int(pad),
                ctypes.cast(stats[0], ctypes.c_void_p), ctypes.cast(stats[1], ctypes.c_void_p),
                flags, b, hb, wb, float(p), int(seed), int(step), int(object_offset))
    return out, chosen


# ------------------------------------------------------------------------------- resampling
def flow_downsample(flow: Tensor, out0: Chan, h: int, w: int, value_scale: float,
                    out1: Optional[Chan] = None, mask: Optional[Tensor] = None,
                    outm: Optional[Chan] = None) -> None:
    """``mask`` ([n·h·w]) / ``outm`` (scflow_flow_downsample_masked): ``out0`` keeps the unmasked
    flow, ``out1`` and ``outm`` receive flow · mask."""
    _require(flow, "flow")
    n, _, H, W = flow.shape
    if mask is not None or outm is not None:
        if mask is not None:
            _require_mask(mask, n * h * w, flow)
        _launch("scflow_flow_downsample_masked", flow, _p(flow), out0.ptr, out0.stride,
                None if out1 is None else out1.ptr, 0 if out1 is None else out1.stride, _p(mask),
                None if outm is None else outm.ptr, 0 if outm is None else outm.stride, n, H, W, h,
                w, float(value_scale))
        return
    _launch("scflow_flow_downsample", flow,
        _p(flow), out0.ptr, out0.stride, None if out1 is None else out1.ptr,
        0 if out1 is None else out1.stride, n, H, W, h, w, float(value_scale))


def flow_upsample(lr: Tensor, delta: Optional[Tensor], mask: Optional[Tensor], n: int, h: int,
                  w: int, H: int, W: int, value_scale: float, flow_out: Tensor,
                  mask_out: Optional[Tensor]) -> None:
    _require(lr, "lr flow")
    _launch("scflow_flow_upsample", lr,_p(lr), _p(delta), _p(mask), _p(flow_out), _p(mask_out),
                                           n, h, w, H, W, float(value_scale))


def convex_upsample(logits: Chan, lr: Tensor, delta: Optional[Tensor], occ: Optional[Tensor],
                    n: int, h: int, w: int, flow_out: Tensor, occ_out: Optional[Tensor] = None,
                    next0: Optional[Chan] = None, next1: Optional[Chan] = None,
                    logit_scale: float = 0.25, value_scale: float = 8.0, scale: int = 8,
                    grid_side: int = 3) -> None:
    """RAFT's convex upsampling (scflow_convex_upsample): ``logits`` channels-last [n·h·w, 576]
    (a ``Chan``), ``lr`` / ``delta`` [n·h·w, 2], ``occ`` [n·h·w, 1] (or None) →
    ``flow_out`` [n, 2, 8h, 8w] = value_scale · Σ softmax(logit_scale · logits) · (lr + delta) over
    the 3×3 neighbourhood, ``occ_out`` [n, 1, 8h, 8w] likewise (no scale); ``next0`` / ``next1``
    receive lr + delta (the next iteration's flow; they must not alias ``lr`` / ``delta``)."""
    _require(logits.buf, "logits")
    _require(lr, "lr flow")
    _require(flow_out, "flow_out")
    m = n * h * w
    if logits.c != grid_side * grid_side * scale * scale:
        raise ValueError(f"convex upsampling expects {grid_side * grid_side * scale * scale} logit "
                         f"channels, got {logits.c}")
    if logits.buf.numel() < m * logits.stride or lr.numel() != 2 * m or \
            (delta is not None and delta.numel() != 2 * m) or (occ is not None and occ.numel() != m):
        raise ValueError("convex_upsample: inputs do not have n·h·w pixels")
    if tuple(flow_out.shape) != (n, 2, scale * h, scale * w) or \
            (occ is not None and (occ_out is None or
                                  tuple(occ_out.shape) != (n, 1, scale * h, scale * w))):
        raise ValueError("convex_upsample: outputs must be [n, 2, 8h, 8w] and [n, 1, 8h, 8w]")
    for nm, c in (("next0", next0), ("next1", next1)):
        if c is not None and (c.c != 2 or c.buf.numel() < m * c.stride):
            raise ValueError(f"convex_upsample: {nm} must be 2 channels of an n·h·w-pixel buffer")
    if delta is not None:
        _require(delta, "delta flow")
    if occ is not None:
        _require(occ, "occlusion")
        _require(occ_out, "occ_out")
    _launch("scflow_convex_upsample", lr, logits.ptr, logits.stride, _p(lr), _p(delta), _p(occ),
            _p(flow_out), _p(occ_out) if occ is not None else None,
            None if next0 is None else next0.ptr, 0 if next0 is None else next0.stride,
            None if next1 is None else next1.ptr, 0 if next1 is None else next1.stride,
            n, h, w, scale, grid_side, float(logit_scale), float(value_scale))


def convex_upsample_backward(logits: Chan, x: Tensor, occ: Optional[Tensor], g_flow: Tensor,
                             g_occ: Optional[Tensor], n: int, h: int, w: int,
                             dlogits: Optional[Chan] = None, logit_scale: float = 0.25,
                             value_scale: float = 8.0, scale: int = 8, grid_side: int = 3
                             ) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """The adjoint of ``convex_upsample`` (scflow_convex_upsample_bwd): ``logits`` channels-last
    [n·h·w, 576] (a ``Chan``), ``x`` [n·h·w, 2] the flow that was upsampled, ``occ`` [n·h·w, 1] or
    None, ``g_flow`` [n, 2, 8h, 8w] and ``g_occ`` [n, 1, 8h, 8w] (or None: a zero gradient) →
    (dlogits [n·h·w, 576] — or the buffer of the given ``Chan``, whose other channels are left
    alone —, dx [n·h·w, 2], docc [n·h·w, 1] or None without ``occ``).  Bitwise reproducible."""
    _require(logits.buf, "logits")
    _require(x, "flow")
    _require(g_flow, "g_flow")
    m = n * h * w
    taps = grid_side * grid_side * scale * scale
    if logits.c != taps:
        raise ValueError(f"convex upsampling expects {taps} logit channels, got {logits.c}")
    if logits.buf.numel() < m * logits.stride or x.numel() != 2 * m or \
            (occ is not None and occ.numel() != m):
        raise ValueError("convex_upsample_backward: inputs do not have n·h·w pixels")
    if tuple(g_flow.shape) != (n, 2, scale * h, scale * w) or \
            (g_occ is not None and tuple(g_occ.shape) != (n, 1, scale * h, scale * w)):
        raise ValueError("convex_upsample_backward: gradients must be [n, 2, 8h, 8w] and "
                         "[n, 1, 8h, 8w]")
    if g_occ is not None and occ is None:
        raise ValueError("convex_upsample_backward: g_occ without occ")
    if occ is not None:
        _require(occ, "occlusion")
    if g_occ is not None:
        _require(g_occ, "g_occ")
    if dlogits is None:
        dlogits = Chan.whole(torch.empty(m, taps, device=x.device, dtype=torch.float32))
    else:
        _require(dlogits.buf, "dlogits")
        if dlogits.c != taps or dlogits.buf.numel() < m * dlogits.stride:
            raise ValueError(f"convex_upsample_backward: dlogits must be {taps} channels of an "
                             "n·h·w-pixel buffer")
    dx = torch.empty(m, 2, device=x.device, dtype=torch.float32)
    docc = None if occ is None else torch.empty(m, 1, device=x.device, dtype=torch.float32)
    ws = torch.empty(m * grid_side * grid_side * 3, device=x.device, dtype=torch.float32)
    _launch("scflow_convex_upsample_bwd", x, logits.ptr, logits.stride, _p(x), _p(occ), _p(g_flow),
            _p(g_occ), dlogits.ptr, dlogits.stride, _p(dx), _p(docc), _p(ws), ws.numel() * 4, n, h, w,
            scale, grid_side, float(logit_scale), float(value_scale))
    return dlogits.buf, dx, docc


def flow_add(lr: Tensor, delta: Tensor, out0: Chan, n: int, h: int, w: int,
             out1: Optional[Chan] = None) -> None:
    """out0 (and out1) ← lr + delta, channels-last [n·h·w, 2] (scflow_flow_add)."""
    _require(lr, "lr flow")
    _require(delta, "delta flow")
    m = n * h * w
    if lr.numel() != 2 * m or delta.numel() != 2 * m or out0.c != 2 or \
            out0.buf.numel() < m * out0.stride or \
            (out1 is not None and (out1.c != 2 or out1.buf.numel() < m * out1.stride)):
        raise ValueError("flow_add: operands must be 2 channels of n·h·w pixels")
    _launch("scflow_flow_add", lr, _p(lr), _p(delta), out0.ptr, out0.stride,
            None if out1 is None else out1.ptr, 0 if out1 is None else out1.stride, n, h, w)


# ------------------------------------------------------------------------------- layout
def nchw_into(x: Tensor, dst: Chan) -> None:
    """x [N,C,H,W] → channels [off, off+C) of channels-last ``dst.buf`` ([N,H,W,Ct] or [NHW,Ct])."""
    _require(x, "x")
    n, c, h, w = x.shape
    if c != dst.c:
        raise ValueError(f"channel mismatch {c} vs {dst.c}")
    st = dst.stride
    _launch("scflow_transpose", x,_p(x), dst.ptr, n, c, h * w, c * h * w, h * w,
                                       h * w * st, st)


def chan_to_nchw(src: Chan, n: int, h: int, w: int, out: Optional[Tensor] = None) -> Tensor:
    res = out if out is not None else torch.empty(n, src.c, h, w, device=src.buf.device,
                                                   dtype=torch.float32)
    st = src.stride
    _launch("scflow_transpose", src.buf,src.ptr, _p(res), n, h * w, src.c, h * w * st, st,
                                       src.c * h * w, h * w)
    return res


# ------------------------------------------------------------------------------- a7 pose head
def ph_conv_pack(weight: Tensor) -> Tensor:
    _require(weight, "pose conv weight", contiguous=False)
    w = weight.detach().contiguous().float()
    cout, cin, kh, kw = w.shape
    lib = _lib.load()
    packed = torch.empty(lib.scflow_ph_conv_packed_size(cout, cin, kh, kw), device=w.device)
    check(lib.scflow_ph_conv_pack(_p(w), _p(packed), cout, cin, kh, kw, _stream(w)),
          "scflow_ph_conv_pack")
    return packed


def ph_conv(src0: Chan, src1: Optional[Chan], packed: Tensor, bias: Optional[Tensor], n: int, h: int,
            w: int, cout: int, k: int, stride: int, pad: int, out: Tensor,
            scale: Optional[Tensor] = None, shift: Optional[Tensor] = None, ksplit: int = 1) -> None:
    """ksplit > 1: ``out`` holds ksplit partial slabs [ksplit, n·oh·ow, cout] (bias None)."""
    _launch("scflow_ph_conv_split", out,
        src0.ptr, src0.c, src0.stride, None if src1 is None else src1.ptr,
        0 if src1 is None else src1.c, 0 if src1 is None else src1.stride, _p(scale), _p(shift),
        _p(packed), _p(bias), _p(out), n, h, w, cout, k, k, stride, pad, ksplit)


def ph_gn_stats(x: Tensor, n: int, hw: int, c: int, groups: int, gamma: Tensor, beta: Tensor,
                eps: float, scale: Tensor, shift: Tensor) -> None:
    _launch("scflow_ph_gn_stats", x,_p(x), n, hw, c, groups, _p(gamma), _p(beta), float(eps),
                                         _p(scale), _p(shift))


def ph_gn_reduce(parts: Tensor, nsplit: int, y: Tensor, n: int, hw: int, c: int, groups: int,
                 gamma: Tensor, beta: Tensor, eps: float, scale: Tensor, shift: Tensor) -> None:
    """y = sum of the nsplit partial slabs of ``parts`` [nsplit, n·hw, c]; GN scale/shift of y."""
    _launch("scflow_ph_gn_reduce", parts,_p(parts), nsplit, n * hw * c, _p(y), n, hw, c, groups,
                                          _p(gamma), _p(beta), float(eps), _p(scale), _p(shift))


def ph_fc_permute(W: Tensor, c: int, hw: int) -> Tensor:
    """nn.Linear weight with NCHW-flatten columns → channels-last column order."""
    _require(W, "fc weight", contiguous=False)
    W = W.detach().contiguous().float()
    Wp = torch.empty_like(W)
    _launch("scflow_ph_fc_permute", W,_p(W), _p(Wp), W.shape[0], c, hw)
    return Wp


def ph_fc(x: Tensor, ldx: int, m: int, k: int, W: Tensor, bias: Optional[Tensor], y: Tensor, n: int,
          relu: bool, gn_c: int = 0, scale: Optional[Tensor] = None,
          shift: Optional[Tensor] = None) -> None:
    _launch("scflow_ph_fc", x,_p(x), ldx, m, k, _p(W), _p(bias), _p(y), n, int(relu), gn_c,
                                   _p(scale), _p(shift))


def ph_fc_split(x: Tensor, ldx: int, m: int, k: int, W: Tensor, parts: Tensor, n: int, ksplit: int,
                gn_c: int = 0, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
                xsplit: int = 0, xbias: Optional[Tensor] = None) -> None:
    """parts [ksplit, m, n] = K-split partial sums of x·Wᵀ (no bias / activation); xsplit > 0:
    x is [xsplit, m, ldx] partial sums read as relu(Σ + xbias)."""
    _launch("scflow_ph_fc_split", x, _p(x), ldx, m, k, _p(W), _p(parts), n, ksplit, gn_c,
            _p(scale), _p(shift), xsplit, _p(xbias))


def ph_fc_sum(parts: Tensor, nsplit: int, m: int, k: int, xbias: Tensor, W: Tensor,
              bias: Optional[Tensor], y: Tensor, n: int, relu: bool) -> None:
    """y = act(relu(Σ parts + xbias)·Wᵀ + bias)."""
    _launch("scflow_ph_fc_sum", parts,_p(parts), nsplit, m, k, _p(xbias), _p(W), _p(bias), _p(y), n,
                                       int(relu))


def ph_heads(x: Tensor, m: int, k: int, Wr: Tensor, br: Tensor, rch: int, Wt: Tensor, bt: Tensor,
             label: Tensor, num_class: int, drot: Tensor, dt: Tensor, xsplit: int = 0,
             xbias: Optional[Tensor] = None) -> None:
    """xsplit > 0: x is [xsplit, m, k] partial sums of the previous FC, read as relu(Σ + xbias)."""
    if label.dtype != torch.int64 or label.device != x.device:
        raise TypeError("label must be an int64 tensor on the same device")
    _launch("scflow_ph_heads_sum", x, _p(x), xsplit, _p(xbias), m, k, _p(Wr), _p(br), rch, _p(Wt),
            _p(bt), _p(label), num_class, _p(drot), _p(dt))


# ------------------------------------------------------------------------------- §8(f)-1 encoder
def enc_conv_pack(weight: Tensor) -> Tensor:
    _require(weight, "encoder conv weight", contiguous=False)
    w = weight.detach().contiguous().float()
    cout, cin, kh, kw = w.shape
    lib = _lib.load()
    size = lib.scflow_enc_conv_packed_size(cout, cin, kh, kw)
    if size < 0:
        check(int(size), "scflow_enc_conv_packed_size")
    packed = torch.empty(size, device=w.device)
    check(lib.scflow_enc_conv_pack(_p(w), _p(packed), cout, cin, kh, kw, _stream(w)),
          "scflow_enc_conv_pack")
    return packed


def enc_stem_pack(weight: Tensor) -> Tensor:
    _require(weight, "encoder stem weight", contiguous=False)
    w = weight.detach().contiguous().float()
    cout, cin, kh, kw = w.shape
    lib = _lib.load()
    packed = torch.empty(lib.scflow_enc_stem_packed_size(cout, cin, kh, kw), device=w.device)
    check(lib.scflow_enc_stem_pack(_p(w), _p(packed), cout, cin, kh, kw, _stream(w)),
          "scflow_enc_stem_pack")
    return packed


def enc_conv(src, packed: Tensor, bias: Optional[Tensor], n: int, h: int, w: int, cin: int,
             cout: int, k: int, stride: int, pad: int, out: Tensor,
             in_scale: Optional[Tensor] = None, in_shift: Optional[Tensor] = None,
             out_scale: Optional[Tensor] = None, out_shift: Optional[Tensor] = None,
             res: Optional[Tensor] = None, act: Optional[str] = None, act2: Optional[str] = None,
             act_split: Optional[int] = None, src1: Optional[Chan] = None, ksplit: int = 1) -> None:
    """One channels-last MFMA conv (see scflow_enc_conv in include/scflow_hip.h); ``src`` is a
    contiguous channels-last tensor or a ``Chan`` (channel slice with its pixel stride)."""
    if isinstance(src, Chan):
        _require(src.buf, "src")
        sptr, sstride = src.ptr, src.stride
    else:
        _require(src, "src")
        sptr, sstride = src.data_ptr(), src.shape[-1]
    _require(out, "out")
    a = _lib.EncConvArgs()
    a.src, a.cin, a.s_in = sptr, cin, sstride
    if src1 is not None:
        _require(src1.buf, "src1")
        a.src1, a.cin1, a.s_in1 = src1.ptr, src1.c, src1.stride
    a.ksplit = ksplit
    a.in_scale, a.in_shift = _p(in_scale), _p(in_shift)
    a.weight, a.bias = packed.data_ptr(), _p(bias)
    a.out_scale, a.out_shift = _p(out_scale), _p(out_shift)
    a.res, a.s_res = _p(res), (res.shape[-1] if res is not None else 0)
    a.out, a.s_out = out.data_ptr(), out.shape[-1]
    a.n, a.h, a.w, a.cout, a.kh, a.kw, a.stride, a.pad = n, h, w, cout, k, k, stride, pad
    a.act = _lib.SCFLOW_ACT[act]
    a.act2 = _lib.SCFLOW_ACT[act2 if act2 is not None else act]
    a.act_split = cout if act_split is None else act_split
    _launch("scflow_enc_conv", out,ctypes.byref(a))


def enc_stem(img: Tensor, packed: Tensor, bias: Optional[Tensor], cout: int, k: int, stride: int,
             pad: int, out: Tensor, out_scale: Optional[Tensor] = None,
             out_shift: Optional[Tensor] = None, act: Optional[str] = None) -> None:
    _require(img, "image")
    n, cin, h, w = img.shape
    _launch("scflow_enc_stem", img,_p(img), _p(packed), _p(bias), _p(out_scale), _p(out_shift),
                                      _p(out), n, cin, h, w, cout, k, k, stride, pad,
                                      _lib.SCFLOW_ACT[act])


def enc_instance_norm_stats(x: Tensor, n: int, hw: int, c: int, scale: Tensor, shift: Tensor,
                            eps: float = 1e-5, partial: Optional[Tensor] = None) -> None:
    """InstanceNorm2d(affine=False) statistics of channels-last x → per (image, channel) affine."""
    chunks = max(1, min(64, hw // 256))
    need = n * chunks * 2 * c
    if partial is None or partial.numel() < need:
        partial = torch.empty(need, dtype=torch.float64, device=x.device)
    lib = _lib.load()
    check(lib.scflow_enc_stats(_p(x), n, hw, c, chunks, _p(partial), _stream(x)), "scflow_enc_stats")
    check(lib.scflow_enc_norm_finalize(_p(partial), n, chunks, c, hw, float(eps), _p(scale),
                                       _p(shift), _stream(x)), "scflow_enc_norm_finalize")


def in_apply(x: Tensor, scale: Tensor, shift: Tensor, y: Tensor, n: int, hw: int, c: int,
             relu: bool) -> None:
    """y = act(x·scale + shift) per (image, channel) of channels-last x (scflow_in_apply)."""
    _launch("scflow_in_apply", x, _p(x), _p(scale), _p(shift), _p(y), n, hw, c, int(bool(relu)))


def in_backward(dy: Tensor, x: Tensor, scale: Tensor, shift: Tensor, dx: Tensor, n: int, hw: int,
                c: int, relu: bool) -> None:
    """InstanceNorm(+ReLU) backward (scflow_in_backward): dx from dy, the input x and its
    scale/shift (rstd, −mean·rstd)."""
    chunks = max(1, min(64, hw // 256))
    partial = torch.empty(n * chunks * 2 * c, dtype=torch.float64, device=x.device)
    mm = torch.empty(n * 2 * c, device=x.device)
    _launch("scflow_in_backward", x, _p(dy), _p(x), _p(scale), _p(shift), _p(dx), _p(partial),
            _p(mm), n, hw, c, chunks, int(bool(relu)))


def _bn_chunks(m: int) -> int:
    return max(1, min(1024, m // 256))


def bn_forward(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], y: Tensor,
               running_mean: Optional[Tensor], running_var: Optional[Tensor], eps: float,
               momentum: float, relu: bool, res: Optional[Tensor] = None
               ) -> Tuple[Tensor, Tensor]:
    """BatchNorm2d (train mode) of channels-last x [..., c] (+ReLU, + res before the ReLU) into y,
    running statistics updated in place (scflow_bn_forward).  Returns (rstd, shift) per channel
    (x̂ = x·rstd + shift) for the backward."""
    c = x.shape[-1]
    m = x.numel() // c
    chunks = _bn_chunks(m)
    dev = x.device
    rstd, shift = torch.empty(c, device=dev), torch.empty(c, device=dev)
    sc, sh = torch.empty(c, device=dev), torch.empty(c, device=dev)
    partial = torch.empty(chunks * 2 * c, dtype=torch.float64, device=dev)
    _launch("scflow_bn_forward", x, _p(x), _p(gamma), _p(beta), _p(res), _p(y), _p(running_mean),
            _p(running_var), _p(rstd), _p(shift), _p(sc), _p(sh), _p(partial), m, c, chunks,
            float(eps), float(momentum), int(bool(relu)))
    return rstd, shift


def bn_backward(dy: Tensor, x: Tensor, rstd: Tensor, shift: Tensor, gamma: Optional[Tensor],
                beta: Optional[Tensor], dx: Tensor, dgamma: Optional[Tensor],
                dbeta: Optional[Tensor], relu: bool, y: Optional[Tensor] = None,
                dres: Optional[Tensor] = None, accumulate: bool = False) -> None:
    """BatchNorm2d (train mode) backward (scflow_bn_backward); y / dres: the residual form (ReLU
    mask from the block output, the identity's gradient written to dres)."""
    c = x.shape[-1]
    m = x.numel() // c
    chunks = _bn_chunks(m)
    partial = torch.empty(chunks * 2 * c, dtype=torch.float64, device=x.device)
    mm = torch.empty(2 * c, device=x.device)
    _launch("scflow_bn_backward", x, _p(dy), _p(x), _p(rstd), _p(shift), _p(gamma), _p(beta), _p(y),
            _p(dx), _p(dres), _p(dgamma), _p(dbeta), _p(partial), _p(mm), m, c, chunks,
            int(bool(relu)), int(bool(accumulate)))


def colsum(x: Tensor, out: Tensor, accumulate: bool = False) -> Tensor:
    """out (+)= x.sum(0) of a 2-D row-major x with unit column stride (scflow_colsum)."""
    _require(out, "out")
    _require(x, "x", contiguous=False)
    if x.dim() != 2 or x.stride(1) != 1 or out.numel() != x.shape[1]:
        raise ValueError(f"colsum: 2-D row-major x and a [{x.shape[-1]}] out expected")
    rows, cols = x.shape
    lib = _lib.load()
    nws = int(lib.scflow_colsum_workspace(rows, cols))
    ws = torch.empty(max(1, nws), device=x.device) if nws > 0 else None
    check(lib.scflow_colsum(_p(x), rows, cols, x.stride(0), _p(out), int(accumulate), _p(ws),
                            _stream(x)), "scflow_colsum")
    return out


def in_apply_residual(x: Tensor, scale: Tensor, shift: Tensor, res: Tensor, y: Tensor, n: int,
                      hw: int, c: int) -> None:
    """y = relu(x·scale + shift + res) (scflow_in_apply_residual: a residual block's tail)."""
    _require(res, "res")
    _launch("scflow_in_apply_residual", x, _p(x), _p(scale), _p(shift), _p(res), _p(y), n, hw, c)


def in_backward_residual(dy: Tensor, x: Tensor, scale: Tensor, shift: Tensor, y: Tensor,
                         dx: Tensor, dres: Tensor, n: int, hw: int, c: int) -> None:
    """Backward of y = relu(IN(x) + res) (scflow_in_backward_residual): dres = dy·(y > 0), dx
    the InstanceNorm backward of it."""
    chunks = max(1, min(64, hw // 256))
    partial = torch.empty(n * chunks * 2 * c, dtype=torch.float64, device=x.device)
    mm = torch.empty(n * 2 * c, device=x.device)
    _launch("scflow_in_backward_residual", x, _p(dy), _p(x), _p(scale), _p(shift), _p(y), _p(dx),
            _p(dres), _p(partial), _p(mm), n, hw, c, chunks)


def enc_apply(x: Tensor, scale: Tensor, shift: Tensor, out: Tensor, n: int, hw: int, c: int,
              id: Optional[Tensor] = None, id_scale: Optional[Tensor] = None,
              id_shift: Optional[Tensor] = None) -> None:
    _launch("scflow_enc_apply", x,_p(x), _p(scale), _p(shift), _p(id), _p(id_scale),
                                       _p(id_shift), _p(out), n, hw, c)


# ------------------------------------------------------------------------------- §8(f)-2 training
def conv_wgrad(dy: Tensor, src0, src1: Optional[Chan], dw: Tensor, db: Optional[Tensor], n: int,
               h: int, w: int, kh: int, kw: int, stride: int, ph: int, pw: int,
               accumulate: bool = False) -> None:
    """dw [cout, cin0+cin1, kh, kw] (+)= conv weight gradient; db [cout] (+)= Σ dy (optional).
    dy: [n·oh·ow, cout] contiguous; src0 / src1: channels-last tensors or ``Chan`` slices.
    Raises ScflowError(SCFLOW_EUNSUPPORTED) for shapes outside the kernel's set."""
    a, _, _ = _wgrad_args([dy], [src0], None if src1 is None else [src1], dw, db, n, h, w, kh, kw,
                          stride, ph, pw, accumulate)
    check(_lib.load().scflow_conv_wgrad(ctypes.byref(a), _stream(dw)), "scflow_conv_wgrad")


def _wgrad_args(dys: List[Tensor], src0s: list, src1s: Optional[list], dw: Tensor,
                db: Optional[Tensor], n: int, h: int, w: int, kh: int, kw: int, stride: int,
                ph: int, pw: int, accumulate: bool):
    """(walk, (dys, src0s, src1s) pointer arrays, workspace) of a weight gradient over len(dys)
    segments of n images: the filled WgradArgs of the whole walk (n·segs images at the first
    segment's bases) with the workspace scflow_conv_wgrad_workspace asks for, allocated."""
    segs = len(dys)
    if not 1 <= segs <= 8 or len(src0s) != segs or (src1s is not None and len(src1s) != segs):
        raise ValueError(f"conv_wgrad_batched: 1..8 segments with matching sources, got {segs}")
    _require(dw, "dw")

    def desc(x, nm):
        if isinstance(x, Chan):
            _require(x.buf, nm)
            return x.ptr, x.c, x.stride
        _require(x, nm)
        return x.data_ptr(), x.shape[-1], x.shape[-1]

    d0 = [desc(x, "src0") for x in src0s]
    d1 = [desc(x, "src1") for x in src1s] if src1s is not None else None
    for t in dys:
        _require(t, "dy")
        if t.shape != dys[0].shape:
            raise ValueError("conv_wgrad_batched: segments differ in dY shape")
    if len({d[1:] for d in d0}) != 1 or (d1 is not None and len({d[1:] for d in d1}) != 1):
        raise ValueError("conv_wgrad_batched: segments differ in source channels / strides")
    a = _lib.WgradArgs()
    a.dy, a.sdy = dys[0].data_ptr(), dys[0].shape[-1]
    a.src0, a.cin0, a.s0 = d0[0]
    a.src1, a.cin1, a.s1 = d1[0] if d1 is not None else (None, 0, 0)
    a.dw, a.db = dw.data_ptr(), _p(db)
    a.n, a.h, a.w, a.cout, a.kh, a.kw = n * segs, h, w, dys[0].shape[-1], kh, kw
    a.stride, a.ph, a.pw, a.accumulate = stride, ph, pw, int(accumulate)
    need = ctypes.c_longlong(0)
    check(_lib.load().scflow_conv_wgrad_workspace(ctypes.byref(a), ctypes.byref(need)),
          "scflow_conv_wgrad_workspace")
    ws = torch.empty(max(1, need.value), device=dw.device)
    a.workspace, a.workspace_floats = ws.data_ptr(), need.value
    arr = ctypes.c_void_p * segs
    ptrs = (arr(*[t.data_ptr() for t in dys]), arr(*[d[0] for d in d0]),
            arr(*[d[0] for d in d1]) if d1 is not None else None)
    return a, ptrs, ws


def conv_wgrad_batched(dys: List[Tensor], src0s: list, src1s: Optional[list], dw: Tensor,
                       db: Optional[Tensor], n: int, h: int, w: int, kh: int, kw: int, stride: int,
                       ph: int, pw: int, accumulate: bool = False) -> None:
    """dw (+)= Σ_i weight gradient of segment i (dys[i] with src0s[i] / src1s[i], each n images
    of h×w) in one launch (scflow_conv_wgrad_batched; ≤ 8 equally shaped segments; the Winograd,
    1×1, implicit-GEMM and thin kernels — ScflowError(SCFLOW_EUNSUPPORTED) otherwise)."""
    a, ptrs, _ = _wgrad_args(dys, src0s, src1s, dw, db, n, h, w, kh, kw, stride, ph, pw, accumulate)
    a.n = n  # the launch takes one segment's images
    check(_lib.load().scflow_conv_wgrad_batched(ctypes.byref(a), len(dys), *ptrs, _stream(dw)),
          "scflow_conv_wgrad_batched")


def conv_wgrad_plan(dys: List[Tensor], src0s: list, src1s: Optional[list], dw: Tensor,
                    db: Optional[Tensor], n: int, h: int, w: int, kh: int, kw: int, stride: int,
                    ph: int, pw: int, accumulate: bool = False) -> Tuple[int, int]:
    """scflow_conv_wgrad_plan (host-only) for conv_wgrad_batched's arguments: (the kernel family
    ``_lib.WGRAD_*`` that call launches, the workspace floats it needs); nothing is launched."""
    a, _, _ = _wgrad_args(dys, src0s, src1s, dw, db, n, h, w, kh, kw, stride, ph, pw, accumulate)
    kind, floats = ctypes.c_int(0), ctypes.c_longlong(0)
    check(_lib.load().scflow_conv_wgrad_plan(ctypes.byref(a), len(dys), ctypes.byref(kind),
                                             ctypes.byref(floats)), "scflow_conv_wgrad_plan")
    return kind.value, floats.value


def im2col(x, n: int, h: int, w: int, cin: int, kh: int, kw: int, stride: int, ph: int, pw: int,
           out: Optional[Tensor] = None, channel_major: bool = False) -> Tensor:
    """Patch matrix [n·oh·ow, kh·kw·cin] of a channels-last input (tensor or Chan); columns in
    (ty, tx, c) order, or (c, ty, tx) with channel_major (a conv weight's own order)."""
    if isinstance(x, Chan):
        _require(x.buf, "x")
        ptr, sx, dev = x.ptr, x.stride, x.buf.device
    else:
        _require(x, "x")
        ptr, sx, dev = x.data_ptr(), x.shape[-1], x.device
    oh, ow = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
    if out is None:
        out = torch.empty(n * oh * ow, kh * kw * cin, device=dev)
    check(_lib.load().scflow_im2col_ex(ptr, sx, _p(out), n, h, w, cin, kh, kw, stride, ph, pw,
                                       int(channel_major), torch.cuda.current_stream(dev).cuda_stream),
          "scflow_im2col_ex")
    return out


def pose_update6_train(drot: Tensor, dt: Tensor, R: Tensor, t: Tensor, weight: float, depth_exp: bool,
                       detach_xy: bool, grads: Optional[Tuple[Tensor, Tensor]] = None):
    """Forward (Rn, tn) or, given grads = (gRn, gtn), the backward (g drot, g dt, g R, g t) of the
    training step's ortho6d pose update (scflow_pose_update6_train)."""
    for nm, x in (("drot", drot), ("dt", dt), ("R", R), ("t", t)):
        _require(x, nm)
    n = drot.shape[0]
    if grads is None:
        Rn = torch.empty(n, 3, 3, device=drot.device)
        tn = torch.empty(n, 3, device=drot.device)
        _launch("scflow_pose_update6_train", drot, _p(drot), _p(dt), _p(R), _p(t), None, None, _p(Rn),
                _p(tn), None, None, n, float(weight), int(depth_exp), int(detach_xy), 0)
        return Rn, tn
    gRn, gtn = grads
    out = [torch.empty(n, 6, device=drot.device), torch.empty(n, 3, device=drot.device),
           torch.empty(n, 3, 3, device=drot.device), torch.empty(n, 3, device=drot.device)]
    _launch("scflow_pose_update6_train", drot, _p(drot), _p(dt), _p(R), _p(t), _p(gRn), _p(gtn),
            *[_p(o) for o in out], n, float(weight), int(depth_exp), int(detach_xy), 1)
    return tuple(out)


def pm_loss(pts: Tensor, gt_r: Tensor, gt_t: Tensor, pred_r: Tensor, pred_t: Tensor,
            sym: Optional[Tensor], diam: Tensor, weight: float):
    """Fused point-matching loss of one iteration (scflow_pm_loss): (loss [1], workspace) where
    workspace = (gt_rt, pred_rot, idx) feeds pm_loss_backward."""
    B, P, _ = pts.shape
    for nm, x in (("pts", pts), ("gt_r", gt_r), ("gt_t", gt_t), ("pred_r", pred_r), ("pred_t", pred_t),
                  ("diam", diam)):
        _require(x, nm)
    gt_rt = torch.empty(B, P, 3, device=pts.device)
    pred_rot = torch.empty(B, P, 3, device=pts.device)
    idx = torch.empty(B, P, dtype=torch.int64, device=pts.device) if sym is not None else None
    loss = torch.empty(1, device=pts.device)
    _launch("scflow_pm_loss", pts, _p(pts), _p(gt_r), _p(gt_t), _p(pred_r), _p(pred_t), _p(sym), _p(diam),
            _p(gt_rt), _p(pred_rot), _p(idx), _p(loss), B, P, float(weight))
    return loss, (gt_rt, pred_rot, idx)


def pm_loss_backward(gloss: Tensor, pts: Tensor, ws, sym: Optional[Tensor], pred_t: Tensor,
                     gt_t: Tensor, diam: Tensor, weight: float) -> Tuple[Tensor, Tensor]:
    gt_rt, pred_rot, idx = ws
    B, P, _ = pts.shape
    g_r = torch.empty(B, 3, 3, device=pts.device)
    g_t = torch.empty(B, 3, device=pts.device)
    _launch("scflow_pm_loss_backward", pts, _p(gloss), _p(pts), _p(gt_rt), _p(pred_rot), _p(idx), _p(sym),
            _p(pred_t), _p(gt_t), _p(diam), _p(g_r), _p(g_t), B, P, float(weight))
    return g_r, g_t


def up_l1_loss(f: Tensor, target: Tensor, vmask: Optional[Tensor], sval: float,
               denom: Optional[Tensor], cdenom: float, weight: float) -> Tuple[Tensor, Tensor]:
    """(loss [1], sgn [N, C, H, W]) of scflow_up_l1_loss; f channels-last [N, h, w, C]."""
    _require(f, "f")
    _require(target, "target")
    N, h, w, C = f.shape
    H, W = target.shape[-2:]
    sgn = torch.empty(N, C, H, W, device=f.device)
    partial = torch.empty((N * H * W + 255) // 256, device=f.device)
    loss = torch.empty(1, device=f.device)
    _launch("scflow_up_l1_loss", f, _p(f), C, h, w, _p(target), _p(vmask), N, H, W, float(sval),
            _p(denom), float(cdenom), float(weight), _p(sgn), _p(partial), _p(loss))
    return loss, sgn


def knn1(gt: Tensor, pred: Tensor) -> Tensor:
    """[B, P] int64 index of the nearest ``pred`` point ([B, Q, 3]) of every ``gt`` point ([B, P, 3])."""
    _require(gt, "gt")
    _require(pred, "pred")
    B, P, _ = gt.shape
    idx = torch.empty(B, P, dtype=torch.int64, device=gt.device)
    _launch("scflow_knn1", gt, _p(gt), _p(pred), _p(idx), B, P, pred.shape[1])
    return idx


def pose_err_sym(points: Tensor, counts: Tensor, sym: Tensor, sym_offset: Tensor, labels: Tensor,
                 R_est: Tensor, t_est: Tensor, R_gt: Tensor, t_gt: Tensor, K: Optional[Tensor],
                 want_mssd: bool = True, want_mspd: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """(mssd [N], mspd [N]) of scflow_pose_err_sym (None for the one not asked for): points
    [C, P, 3] / counts [C] int32 (``patches.point_table``), sym [T, 12] / sym_offset [C + 1] int32,
    labels [N] int32, poses [N, 3, 3] / [N, 3], K [N, 3, 3] (needed for mspd)."""
    for nm, t in (("points", points), ("sym", sym), ("R_est", R_est), ("t_est", t_est),
                  ("R_gt", R_gt), ("t_gt", t_gt)) + ((("K", K),) if K is not None else ()):
        _require(t, nm)
    for nm, t in (("counts", counts), ("sym_offset", sym_offset), ("labels", labels)):
        _require(t, nm, dtype=torch.int32)
    C, P, _ = points.shape
    n = labels.shape[0]
    if counts.shape[0] != C or sym_offset.shape[0] != C + 1 or sym.dim() != 2 or sym.shape[1] != 12:
        raise ValueError(f"counts {tuple(counts.shape)}, sym_offset {tuple(sym_offset.shape)}, sym "
                         f"{tuple(sym.shape)} do not fit {C} classes")
    for nm, t, shp in (("R_est", R_est, (n, 3, 3)), ("t_est", t_est, (n, 3)), ("R_gt", R_gt, (n, 3, 3)),
                       ("t_gt", t_gt, (n, 3))) + ((("K", K, (n, 3, 3)),) if K is not None else ()):
        if tuple(t.shape) != shp:
            raise ValueError(f"{nm} must be {shp}, got {tuple(t.shape)}")
    mssd = torch.empty(n, device=points.device) if want_mssd else None
    mspd = torch.empty(n, device=points.device) if want_mspd else None
    _launch("scflow_pose_err_sym", points, _p(points), _p(counts), C, P, _p(sym), _p(sym_offset),
            sym.shape[0], _p(labels), _p(R_est), _p(t_est), _p(R_gt), _p(t_gt), _p(K), _p(mssd),
            _p(mspd), n)
    return mssd, mspd


def vsd_counts(depth_est: Tensor, depth_gt: Tensor, depth_test: Tensor, frame_index: Tensor, K: Tensor,
               diameter: Optional[Tensor], taus: Tensor, delta: float) -> Tensor:
    """counts [N, 2 + n_taus] int32 = (|U|, |I|, cost_k …) of scflow_vsd_counts: depth_est /
    depth_gt [N, H, W], depth_test [F, H, W], frame_index [N] int32, K [N, 3, 3], diameter [N] or
    None (costs not normalised), taus [n_taus]."""
    for nm, t in (("depth_est", depth_est), ("depth_gt", depth_gt), ("depth_test", depth_test),
                  ("K", K), ("taus", taus)) + ((("diameter", diameter),) if diameter is not None else ()):
        _require(t, nm)
    _require(frame_index, "frame_index", dtype=torch.int32)
    n, h, w = depth_est.shape
    if depth_gt.shape != depth_est.shape or depth_test.dim() != 3 or tuple(depth_test.shape[1:]) != (h, w):
        raise ValueError(f"depth maps disagree: est {tuple(depth_est.shape)}, gt {tuple(depth_gt.shape)}, "
                         f"test {tuple(depth_test.shape)}")
    if frame_index.shape[0] != n or tuple(K.shape) != (n, 3, 3) or \
            (diameter is not None and diameter.shape[0] != n):
        raise ValueError("frame_index, K and diameter hold one entry per pair")
    counts = torch.empty(n, 2 + taus.shape[0], dtype=torch.int32, device=depth_est.device)
    _launch("scflow_vsd_counts", depth_est, _p(depth_est), _p(depth_gt), _p(depth_test),
            _p(frame_index), _p(K), _p(diameter), _p(taus), taus.shape[0], float(delta), _p(counts),
            n, depth_test.shape[0], h, w)
    return counts


SCENE_OUTPUTS = ("stats", "inst_id", "depth_scene", "depth_inst", "mask_visib")


def scene_visibility(verts: Tensor, faces: Tensor, vert_offset: Tensor, face_offset: Tensor,
                     bounds: Tensor, labels: Tensor, frame_index: Tensor, R: Tensor, t: Tensor,
                     K: Tensor, height: int, width: int, depth_test: Optional[Tensor] = None,
                     delta: float = 15.0, margin: Tuple[int, int] = (0, 0), pixel_offset: float = 0.0,
                     want: Sequence[str] = ("stats", "inst_id")) -> Dict[str, Tensor]:
    """scflow_scene_visibility: the mesh table (verts [ΣV, 3], faces [ΣF, 3] int32, vert_offset /
    face_offset [C + 1] int32, bounds [C, 6]), labels / frame_index [n] int32 (frame_index
    non-decreasing), R [n, 3, 3], t [n, 3], K [F, 3, 3], depth_test [F, H, W] or None, margin
    (x, y) → {name: tensor} for the names in ``want`` (``SCENE_OUTPUTS``): stats [n, 12] int32,
    inst_id [F, H, W] int32, depth_scene [F, H, W], depth_inst [n, H, W], mask_visib [n, H, W]
    uint8.  n = 0: the empty scene (inst_id −1, depths 0), nothing launched."""
    for nm, x in (("verts", verts), ("bounds", bounds), ("R", R), ("t", t), ("K", K)) + \
            ((("depth_test", depth_test),) if depth_test is not None else ()):
        _require(x, nm)
    for nm, x in (("faces", faces), ("vert_offset", vert_offset), ("face_offset", face_offset),
                  ("labels", labels), ("frame_index", frame_index)):
        _require(x, nm, dtype=torch.int32)
    want = tuple(want)
    if not want or any(w not in SCENE_OUTPUTS for w in want):
        raise ValueError(f"want = {want!r}: one or more of {SCENE_OUTPUTS}")
    n, F, C = labels.shape[0], K.shape[0], bounds.shape[0]
    H, W = int(height), int(width)
    if vert_offset.shape[0] != C + 1 or face_offset.shape[0] != C + 1 or tuple(bounds.shape) != (C, 6):
        raise ValueError(f"vert_offset {tuple(vert_offset.shape)}, face_offset {tuple(face_offset.shape)}, "
                         f"bounds {tuple(bounds.shape)} do not fit one class count")
    for nm, x, shp in (("frame_index", frame_index, (n,)), ("R", R, (n, 3, 3)), ("t", t, (n, 3)),
                       ("K", K, (F, 3, 3))) + \
            ((("depth_test", depth_test, (F, H, W)),) if depth_test is not None else ()):
        if tuple(x.shape) != shp:
            raise ValueError(f"{nm} must be {shp}, got {tuple(x.shape)}")
    dev = verts.device
    new = {"stats": lambda: torch.empty(n, 12, dtype=torch.int32, device=dev),
           "inst_id": lambda: torch.full((F, H, W), -1, dtype=torch.int32, device=dev) if n == 0
           else torch.empty(F, H, W, dtype=torch.int32, device=dev),
           "depth_scene": lambda: torch.zeros(F, H, W, device=dev) if n == 0
           else torch.empty(F, H, W, device=dev),
           "depth_inst": lambda: torch.empty(n, H, W, device=dev),
           "mask_visib": lambda: torch.empty(n, H, W, dtype=torch.uint8, device=dev)}
    out = {w: new[w]() for w in want}
    a = _lib.SceneArgs()
    a.verts, a.faces, a.vert_offset, a.face_offset = _p(verts), _p(faces), _p(vert_offset), _p(face_offset)
    a.bounds, a.num_classes, a.total_verts, a.total_faces = _p(bounds), C, verts.shape[0], faces.shape[0]
    a.labels, a.frame_index, a.R, a.t, a.K = _p(labels), _p(frame_index), _p(R), _p(t), _p(K)
    a.n, a.n_frames, a.height, a.width = n, F, H, W
    a.margin_x, a.margin_y = int(margin[0]), int(margin[1])
    a.pixel_offset, a.delta = float(pixel_offset), float(delta)
    a.depth_test = _p(depth_test)
    for w in SCENE_OUTPUTS:
        setattr(a, w, _p(out.get(w)))
    _launch("scflow_scene_visibility", verts, ctypes.byref(a))
    return out


FLOW_DEPTH_COMBINE = {"or": _lib.FLOW_DEPTH_OR, "reference": _lib.FLOW_DEPTH_REFERENCE}


def _require_all_contiguous(named) -> None:
    """Contiguity of every given tensor, checked before anything else (device included)."""
    for nm, x, *_ in named:
        if isinstance(x, torch.Tensor) and not x.is_contiguous():
            raise ValueError(f"{nm} must be contiguous")


def _require_plane(t: Tensor, name: str, dtypes, shape: tuple) -> None:
    """A filter's [N, H, W] input of one of ``dtypes`` (the first is the one reported)."""
    if isinstance(t, torch.Tensor) and t.dtype not in dtypes:
        raise TypeError(f"{name} must be one of {dtypes}, got {t.dtype}")
    _require(t, name, dtype=t.dtype if isinstance(t, torch.Tensor) else dtypes[0])
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")


def flow_gt(depth: Optional[Tensor] = None, K: Optional[Tensor] = None, R_ref: Optional[Tensor] = None,
            t_ref: Optional[Tensor] = None, R_gt: Optional[Tensor] = None, t_gt: Optional[Tensor] = None,
            flow_in: Optional[Tensor] = None, invalid_num: float = 400.0,
            gt_mask: Optional[Tensor] = None, depth1: Optional[Tensor] = None, depth_thr: float = 0.2,
            depth_combine: str = "or", face_index1: Optional[Tensor] = None,
            face_index2: Optional[Tensor] = None, want_flow: bool = True, want_filtered: bool = True
            ) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """scflow_flow_gt, one launch: the flow from the poses (depth [N, H, W], K, R_ref, t_ref, R_gt,
    t_gt: the bits of ``lift_points`` + ``pose_flow``) or ``flow_in`` [N, 2, H, W], and the filters
    selected by gt_mask (bool / uint8 / float32), depth1 (with ``depth`` as depth0) and face_index1
    / face_index2 (int32 or int64, both the same) → (flow, filtered flow), None where not wanted.
    Out of place.  Every argument is checked before the launch."""
    poses = (("K", K, (3, 3)), ("R_ref", R_ref, (3, 3)), ("t_ref", t_ref, (3,)),
             ("R_gt", R_gt, (3, 3)), ("t_gt", t_gt, (3,)))
    _require_all_contiguous(poses + (("depth", depth), ("flow_in", flow_in), ("gt_mask", gt_mask),
                                     ("depth1", depth1), ("face_index1", face_index1),
                                     ("face_index2", face_index2)))
    if flow_in is not None:
        if any(x is not None for _, x, _ in poses):
            raise ValueError("flow_gt takes the poses or flow_in, not both")
        if not isinstance(flow_in, torch.Tensor) or flow_in.dim() != 4 or flow_in.shape[1] != 2:
            raise ValueError("flow_in must be a [N, 2, H, W] tensor")
        n, _, h, w = flow_in.shape
        dev = flow_in
    else:
        if depth is None or any(x is None for _, x, _ in poses):
            raise ValueError("flow_gt needs depth, K, R_ref, t_ref, R_gt and t_gt, or flow_in")
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise ValueError("depth must be a [N, H, W] tensor")
        n, h, w = depth.shape
        dev = depth
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"flow_gt: empty input [{n}, {h}, {w}]")
    if flow_in is not None:
        _require(flow_in, "flow_in")
    else:
        for nm, x, shp in poses:
            _require(x, nm)
            if tuple(x.shape) != (n,) + shp:
                raise ValueError(f"{nm} must be {(n,) + shp}, got {tuple(x.shape)}")
    if depth_combine not in FLOW_DEPTH_COMBINE:
        raise ValueError(f"depth_combine = {depth_combine!r}: one of {tuple(FLOW_DEPTH_COMBINE)}")
    if not (want_flow or want_filtered):
        raise ValueError("flow_gt: no output wanted")
    if depth is not None:
        _require_plane(depth, "depth", (torch.float32,), (n, h, w))
    if gt_mask is not None:
        _require_plane(gt_mask, "gt_mask", (torch.bool, torch.uint8, torch.float32), (n, h, w))
    if depth1 is not None:
        if depth is None:
            raise ValueError("the depth filter needs depth (depth0) beside depth1")
        _require_plane(depth1, "depth1", (torch.float32,), (n, h, w))
    if (face_index1 is None) != (face_index2 is None):
        raise ValueError("the face-index filter needs face_index1 and face_index2")
    if face_index1 is not None:
        _require_plane(face_index1, "face_index1", (torch.int32, torch.int64), (n, h, w))
        _require_plane(face_index2, "face_index2", (face_index1.dtype,), (n, h, w))
    flow = torch.empty(n, 2, h, w, device=dev.device) if want_flow else None
    filt = torch.empty(n, 2, h, w, device=dev.device) if want_filtered else None
    a = _lib.FlowGtArgs()
    a.depth, a.flow_in = _p(depth), _p(flow_in)
    a.K, a.R_ref, a.t_ref, a.R_gt, a.t_gt = _p(K), _p(R_ref), _p(t_ref), _p(R_gt), _p(t_gt)
    a.n, a.h, a.w, a.invalid_num = n, h, w, float(invalid_num)
    a.gt_mask = _p(gt_mask)
    a.mask_dtype = 1 if gt_mask is not None and gt_mask.dtype == torch.float32 else 0
    a.depth1, a.depth_thr, a.depth_combine = _p(depth1), float(depth_thr), FLOW_DEPTH_COMBINE[depth_combine]
    a.face_index1, a.face_index2 = _p(face_index1), _p(face_index2)
    a.face_dtype = 1 if face_index1 is not None and face_index1.dtype == torch.int64 else 0
    a.flow, a.flow_filtered = _p(flow), _p(filt)
    _launch("scflow_flow_gt", dev, ctypes.byref(a))
    return flow, filt


def flow_epe(flow_tgt: Tensor, flow_pred: Tensor, mask: Optional[Tensor] = None,
             max_flow: float = 400.0, threshs: Sequence[float] = (1.0, 3.0, 5.0),
             occ_pred: Optional[Tensor] = None, want_stats: bool = True, want_map: bool = False
             ) -> Tuple[Optional[Tensor], Optional[Tensor], Optional[Tensor]]:
    """scflow_flow_epe: flow_tgt / flow_pred [N, 2, H, W], mask / occ_pred [N, H, W] float32 or None
    → (counts [N, 4] int32 = valid pixels and valid pixels below each of the three thresholds, sums
    [N, 2] float64 = Σ error over valid pixels and Σ |inside − occ_pred| over all pixels, error map
    [N, H, W] or None).  Two launches and no synchronisation; the sums are bitwise reproducible."""
    _require_all_contiguous((("flow_tgt", flow_tgt), ("flow_pred", flow_pred), ("mask", mask),
                             ("occ_pred", occ_pred)))
    if not isinstance(flow_tgt, torch.Tensor) or not isinstance(flow_pred, torch.Tensor) or \
            flow_tgt.dim() != 4 or flow_tgt.shape[1] != 2 or flow_pred.shape != flow_tgt.shape:
        raise ValueError("flow_tgt and flow_pred must be tensors of the same shape [N, 2, H, W]")
    n, _, h, w = flow_tgt.shape
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"flow_epe: empty input [{n}, {h}, {w}]")
    _require(flow_tgt, "flow_tgt")
    _require(flow_pred, "flow_pred")
    for nm, x in (("mask", mask), ("occ_pred", occ_pred)):
        if x is not None:
            _require_plane(x, nm, (torch.float32,), (n, h, w))
    threshs = tuple(float(v) for v in threshs)
    if len(threshs) != 3:
        raise ValueError(f"flow_epe counts under three thresholds, got {threshs}")
    if not (want_stats or want_map):
        raise ValueError("flow_epe: no output wanted")
    dev = flow_tgt.device
    counts = sums = ws = emap = None
    if want_stats:
        counts = torch.empty(n, 4, dtype=torch.int32, device=dev)
        sums = torch.empty(n, 2, dtype=torch.float64, device=dev)
        ws = torch.empty(max(int(_lib.load().scflow_flow_epe_workspace(n, h, w)), 8) // 8,
                         dtype=torch.float64, device=dev)
    if want_map:
        emap = torch.empty(n, h, w, device=dev)
    a = _lib.FlowEpeArgs()
    a.flow_tgt, a.flow_pred, a.mask, a.occ_pred = _p(flow_tgt), _p(flow_pred), _p(mask), _p(occ_pred)
    a.n, a.h, a.w, a.max_flow = n, h, w, float(max_flow)
    a.thresh = (ctypes.c_float * 3)(*threshs)
    a.counts, a.sums, a.err_map = _p(counts), _p(sums), _p(emap)
    a.workspace, a.workspace_bytes = _p(ws), 0 if ws is None else ws.numel() * 8
    _launch("scflow_flow_epe", flow_tgt, ctypes.byref(a))
    return counts, sums, emap


def group_norm_forward(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float,
                       relu: bool) -> Tuple[Tensor, Tensor]:
    """GroupNorm (+ReLU) of channels-last x [n, h, w, c] (c == 4·groups) → (y, stats [n·groups, 2]
    = (mean, rstd))."""
    for nm, t in (("x", x), ("gamma", gamma), ("beta", beta)):
        _require(t, nm)
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    y = torch.empty_like(x)
    stats = torch.empty(n * groups, 2, device=x.device, dtype=torch.float32)
    _launch("scflow_group_norm_forward", x, _p(x), _p(gamma), _p(beta), _p(y), _p(stats), n, hw, c,
            groups, float(eps), int(relu))
    return y, stats


def group_norm_backward(dy: Tensor, x: Tensor, gamma: Tensor, beta: Tensor, stats: Tensor,
                        groups: int, relu: bool, dgamma: Tensor, dbeta: Tensor,
                        accumulate: bool) -> Tensor:
    """dx of group_norm_forward; dγ / dβ written to (or, accumulate, added onto) dgamma / dbeta."""
    for nm, t in (("dy", dy), ("x", x), ("gamma", gamma), ("beta", beta), ("stats", stats),
                  ("dgamma", dgamma), ("dbeta", dbeta)):
        _require(t, nm)
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    dx = torch.empty_like(x)
    part = torch.empty(n * c * 2, device=x.device, dtype=torch.float32)
    _launch("scflow_group_norm_backward", x, _p(dy), _p(x), _p(gamma), _p(beta), _p(stats), _p(dx),
            _p(part), _p(dgamma), _p(dbeta), n, hw, c, groups, int(relu), int(accumulate))
    return dx


def gru_gate_forward(zr: Tensor, h: Tensor, out: Tensor, q: Optional[Tensor] = None) -> Tensor:
    """SepConvGRU gate (training): out = r·h (q None) or h + z·(q − h); zr [..., 2c], h / q / out
    [..., c], channels-last contiguous."""
    for nm, t in (("zr", zr), ("h", h), ("out", out)) + ((("q", q),) if q is not None else ()):
        _require(t, nm)
    c = h.shape[-1]
    _launch("scflow_gru_gate_forward", h, _p(zr), _p(h), _p(q), _p(out), h.numel() // c, c,
            0 if q is None else 1)
    return out


def gru_gate_backward_q(dh2: Tensor, zr: Tensor, h: Tensor, q: Tensor, dq: Tensor, dzr: Tensor,
                        dha: Tensor) -> None:
    """dq = dh2·z·(1 − q²), dzr[..., :c] = dh2·(q − h)·z(1 − z), dha = dh2·(1 − z); dh2 may be
    a channel slice (pixel stride ≥ c)."""
    for nm, t in (("zr", zr), ("h", h), ("q", q), ("dq", dq), ("dzr", dzr), ("dha", dha)):
        _require(t, nm)
    _require_rows(dh2, "dh2")
    c = h.shape[-1]
    _launch("scflow_gru_gate_backward_q", h, _p(dh2), dh2.stride(-2), _p(zr), _p(h), _p(q), _p(dq),
            _p(dzr), _p(dha), h.numel() // c, c)


def gru_gate_backward_r(drh: Tensor, zr: Tensor, h: Tensor, dha: Tensor, dzr: Tensor,
                        dh: Tensor) -> None:
    """dzr[..., c:] = drh·h·r(1 − r), dh = dha + drh·r; drh and dh may be channel slices (pixel
    stride ≥ c), and dh may be drh itself (overwritten in place)."""
    for nm, t in (("zr", zr), ("h", h), ("dha", dha), ("dzr", dzr)):
        _require(t, nm)
    _require_rows(drh, "drh")
    _require_rows(dh, "dh")
    c = h.shape[-1]
    _launch("scflow_gru_gate_backward_r", h, _p(drh), drh.stride(-2), _p(zr), _p(h), _p(dha),
            _p(dzr), _p(dh), dh.stride(-2), h.numel() // c, c)


def col2im(cols: Tensor, n: int, h: int, w: int, cin: int, kh: int, kw: int, stride: int, ph: int,
           pw: int, out: Optional[Tensor] = None) -> Tensor:
    """Adjoint of im2col: [n·oh·ow, kh·kw·cin] patch gradients → channels-last [n, h, w, cin]."""
    _require(cols, "cols")
    if out is None:
        out = torch.empty(n, h, w, cin, device=cols.device)
    _require(out, "out", contiguous=False)
    _launch("scflow_col2im", cols, _p(cols), _p(out), out.stride(-2), n, h, w, cin, kh, kw, stride,
            ph, pw)
    return out


def corr_lookup_backward(dout: Tensor, flow: Tensor, dpyr: Tensor, n: int, h: int, w: int,
                         num_levels: int, radius: int, out_layout: str = "nhwc",
                         flow_layout: str = "nhwc", mask: Optional[Tensor] = None) -> None:
    """dpyr (zeroed, pyramid layout) += adjoint of corr_lookup applied to dout; with ``mask``
    ([n·h·w]) to mask · dout (scflow_corr_lookup_backward_masked; no gradient for the mask)."""
    for nm, t in (("dout", dout), ("flow", flow), ("dpyr", dpyr)):
        _require(t, nm)
    lay = {"nchw": _lib.LAYOUT_NCHW, "nhwc": _lib.LAYOUT_NHWC}
    stride = dout.shape[-1] if out_layout == "nhwc" else 0
    if mask is not None:
        _require_mask(mask, n * h * w, dout)
        _launch("scflow_corr_lookup_backward_masked", dout, _p(dout), lay[out_layout], stride,
                _p(flow), lay[flow_layout], _p(mask), _p(dpyr), n, h, w, num_levels, radius)
        return
    _launch("scflow_corr_lookup_backward", dout,_p(dout), lay[out_layout], stride, _p(flow),
                                                  lay[flow_layout], _p(dpyr), n, h, w, num_levels,
                                                  radius)


def gemm(a: Tensor, b: Tensor, out: Optional[Tensor] = None, alpha: float = 1.0, beta: float = 0.0,
         bias: Optional[Tensor] = None, bias_dim: str = "n") -> Tensor:
    """``alpha·(a @ b) [+ beta·out] [+ bias]`` on the HIP fp32 MFMA GEMM (scflow_gemm_f32).
    ``a`` [M, K] or [Bt, M, K], ``b`` [K, N] or [Bt, K, N] — any strides (transposed views are
    free); ``out`` [M, N] / [Bt, M, N] (any strides; allocated contiguous if None; read when
    beta ≠ 0).  ``bias`` [N] (bias_dim "n") or [M] ("m")."""
    for t, nm in ((a, "a"), (b, "b")):
        _require(t, nm, contiguous=False)
    batched = a.dim() == 3
    if a.dim() != b.dim() or a.dim() not in (2, 3):
        raise ValueError(f"gemm: a {tuple(a.shape)} and b {tuple(b.shape)} must both be 2-D or 3-D")
    A = a if batched else a.unsqueeze(0)
    B = b if batched else b.unsqueeze(0)
    bt, M, K = A.shape
    if B.shape[0] != bt or B.shape[1] != K:
        raise ValueError(f"gemm: shapes {tuple(a.shape)} x {tuple(b.shape)} do not contract")
    N = B.shape[2]
    if out is None:
        if beta != 0.0:
            raise ValueError("gemm: beta != 0 needs out")
        out = torch.empty((bt, M, N) if batched else (M, N), device=a.device)
    _require(out, "out", contiguous=False)
    C = out if batched else out.unsqueeze(0)
    if tuple(C.shape) != (bt, M, N):
        raise ValueError(f"gemm: out {tuple(out.shape)} is not {(bt, M, N)}")
    mode = 0
    if bias is not None:
        _require(bias, "bias")
        mode = 1 if bias_dim == "n" else 2
        if bias.numel() != (N if mode == 1 else M):
            raise ValueError("gemm: bias size")
    sa, sb, sc = A.stride(), B.stride(), C.stride()
    splits = int(_lib.load().scflow_gemm_f32_splits(bt, M, N, K))
    ws = torch.empty(splits * bt * M * N, device=a.device) if splits > 1 else None
    _launch("scflow_gemm_f32", a, _p(a), _p(b), _p(out), _p(bias), bt, M, N, K,
            sa[0], sa[1], sa[2], sb[0], sb[1], sb[2], sc[0], sc[1], sc[2], float(alpha), float(beta), mode,
            splits, _p(ws))
    return out
