"""NumPy restatement of the patch contract (include/scflow_hip.h scflow_patch_*),
stage by stage as the reference's pipeline runs it — box, crop array, resize, pad, normalise —
not the kernel's fused per-pixel formula.

``dtype=np.float32`` performs every floating-point operation of the contract in fp32, one rounding
per operation in the contract's order (what the kernels compute: bit-exact comparisons use it);
``dtype=np.float64`` is the same definition evaluated in fp64 (what tolerances are measured
against).  All index arithmetic is in Python / int64 integers.

``torch_patches`` is the obvious PyTorch version — one ``interpolate`` per object, after a host
synchronisation to learn the crop sizes — which tools/patch_bench.py times next to the kernels.
"""
import numpy as np

MAX_CROP = 8192


# ------------------------------------------------------------------------------ geometry
def matmul3(a, b, dtype=np.float32):
    """3×3 product, each element summed over its three terms in order, rounded after every
    operation."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    c = np.zeros((3, 3), dtype)
    for i in range(3):
        for j in range(3):
            acc = dtype(a[i, 0] * b[0, j])
            acc = dtype(acc + dtype(a[i, 1] * b[1, j]))
            acc = dtype(acc + dtype(a[i, 2] * b[2, j]))
            c[i, j] = acc
    return c


def project(points, R, t, K, dtype=np.float32):
    """K·(R·X + t) → (x, y, z) arrays; products summed left to right."""
    X = np.asarray(points, dtype)
    R, t, K = np.asarray(R, dtype), np.asarray(t, dtype), np.asarray(K, dtype)
    c = [((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)]
    q = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
    with np.errstate(all="ignore"):
        return q[0] / q[2], q[1] / q[2], q[2]


def sizes(cw, ch, S):
    """(nw, nh, left, top) of a cw × ch crop in an S × S patch, in integers."""
    m = max(cw, ch)
    nw, nh = (2 * cw * S + m) // (2 * m), (2 * ch * S + m) // (2 * m)
    return nw, nh, (S - nw) // 2, (S - nh) // 2


def geom_of(x1, y1, x2, y2, S):
    return (x1, y1, x2, y2) + sizes(x2 - x1 + 1, y2 - y1 + 1, S)


def transform(geom, S, K, dtype=np.float32):
    """(T, k) of a geometry: T = T_pad·T_scale·T_crop, k = T·K."""
    x1, y1, x2, y2, nw, nh, left, top = (int(v) for v in geom)
    m = max(x2 - x1 + 1, y2 - y1 + 1)
    sf = dtype(dtype(S) / dtype(m))
    Tc = np.array([[1, 0, -x1], [0, 1, -y1], [0, 0, 1]], dtype)
    Ts = np.array([[sf, 0, 0], [0, sf, 0], [0, 0, 1]], dtype)
    Tp = np.array([[1, 0, left], [0, 1, top], [0, 0, 1]], dtype)
    T = matmul3(matmul3(Tp, Ts, dtype), Tc, dtype)
    return T, matmul3(T, K, dtype)


def boxes(points, R, t, K, ratio, H, W, S, dtype=np.float32, frame_ok=True):
    """One object: dict(bbox, edges, geom, T, k, valid).  ``edges`` are the four crop edges before
    truncation (xc − half, yc − half, xc + half, yc + half)."""
    K = np.asarray(K, dtype)
    x, y, z = project(points, R, t, K, dtype)
    out = dict(geom=(0,) * 8, T=np.eye(3, dtype=dtype), k=K.copy(), valid=False, edges=None)
    if len(x) == 0:
        out["bbox"] = np.array([np.inf, np.inf, -np.inf, -np.inf], dtype)
        return out
    l, tp, r, b = x.min(), y.min(), x.max(), y.max()
    out["bbox"] = bbox = np.array([l, tp, r, b], dtype)
    if not frame_ok or (z <= 0).any() or not np.isfinite(z).all() or not np.isfinite(bbox).all() \
            or not (np.isfinite(x).all() and np.isfinite(y).all()):
        return out
    side = max(dtype(r - l), dtype(b - tp))
    xc, yc = dtype(dtype(l + r) / dtype(2)), dtype(dtype(tp + b) / dtype(2))
    sr = dtype(side * dtype(ratio))
    half = dtype(sr / dtype(2))
    out["edges"] = e = [dtype(xc - half), dtype(yc - half), dtype(xc + half), dtype(yc + half)]
    if not np.isfinite(sr) or sr < 1 or max(abs(v) for v in e) >= 2 ** 20:
        return out
    x1, y1, x2, y2 = (int(v) for v in e)  # int() truncates toward zero
    cw, ch = x2 - x1 + 1, y2 - y1 + 1
    if max(cw, ch) > MAX_CROP or x2 < 0 or y2 < 0 or x1 > W - 1 or y1 > H - 1:
        return out
    out["geom"] = g = geom_of(x1, y1, x2, y2, S)
    out["T"], out["k"] = transform(g, S, K, dtype)
    out["valid"] = True
    return out


# ------------------------------------------------------------------------------ the stages
def crop(frame, x1, y1, x2, y2, pad, dtype=np.float32):
    """mmcv imcrop with an inclusive box: frame [H, W, C] → [ch, cw, C], ``pad`` outside."""
    H, W, C = frame.shape
    out = np.full((y2 - y1 + 1, x2 - x1 + 1, C), pad, dtype)
    ya, yb, xa, xb = max(y1, 0), min(y2, H - 1), max(x1, 0), min(x2, W - 1)
    if ya <= yb and xa <= xb:
        out[ya - y1:yb - y1 + 1, xa - x1:xb - x1 + 1] = frame[ya:yb + 1, xa:xb + 1]
    return out


def linear_coords(n, no, dtype=np.float32):
    """cv2 INTER_LINEAR along one axis, n source → no output samples: (i0, i1, f) per output
    index from the exact rational ((2·o + 1)·n − no) / (2·no)."""
    o = np.arange(no, dtype=np.int64)
    num, den = (2 * o + 1) * n - no, 2 * no
    i0 = num // den
    f = (num - i0 * den).astype(dtype) / dtype(den)
    low, high = i0 < 0, i0 >= n - 1
    i0 = np.where(low, 0, np.where(high, n - 1, i0))
    f = np.where(low | high, dtype(0), f).astype(dtype)
    return i0, np.minimum(i0 + 1, n - 1), f


def resize_linear(img, nw, nh, dtype=np.float32):
    """[ch, cw, C] → [nh, nw, C]; no antialiasing."""
    ch, cw, _ = img.shape
    img = img.astype(dtype)
    x0, x1, fx = linear_coords(cw, nw, dtype)
    y0, y1, fy = linear_coords(ch, nh, dtype)
    fx, fy = fx[None, :, None], fy[:, None, None]
    gx, gy = dtype(1) - fx, dtype(1) - fy
    a, b = img[y0][:, x0], img[y0][:, x1]
    c, d = img[y1][:, x0], img[y1][:, x1]
    up = gx * a + fx * b
    dn = gx * c + fx * d
    return (gy * up + fy * dn).astype(dtype)


def resize_nearest(img, nw, nh):
    ch, cw, _ = img.shape
    sx = np.minimum(np.arange(nw, dtype=np.int64) * cw // nw, cw - 1)
    sy = np.minimum(np.arange(nh, dtype=np.int64) * ch // nh, ch - 1)
    return img[sy][:, sx]


def pad_center(img, S, left, top, pad, dtype=np.float32):
    out = np.full((S, S, img.shape[2]), pad, dtype)
    out[top:top + img.shape[0], left:left + img.shape[1]] = img
    return out


def normalize(img, mean, std, to_rgb, dtype=np.float32):
    """mmcv imnormalize: reverse the channels first, then (v − mean) / std in output order →
    planar [C, S, S]."""
    if to_rgb:
        img = img[..., ::-1]
    out = (img.astype(dtype) - np.asarray(mean, dtype)) / np.asarray(std, dtype)
    return np.ascontiguousarray(out.astype(dtype).transpose(2, 0, 1))


def extract(frame, geom, valid, S, pad=128.0, mean=None, std=None, to_rgb=False, quantize=True,
            nearest=False, dtype=np.float32):
    """One patch [C, S, S] of ``frame`` [H, W, C]."""
    C = frame.shape[2]
    mean = [0.0] * C if mean is None else mean
    std = [1.0] * C if std is None else std
    pad = dtype(np.float32(pad))
    if not valid:
        return normalize(np.full((S, S, C), pad, dtype), mean, std, to_rgb, dtype)
    x1, y1, x2, y2, nw, nh, left, top = (int(v) for v in geom)
    c = crop(frame, x1, y1, x2, y2, pad, dtype)
    if nearest:
        r = resize_nearest(c, nw, nh)
    else:
        r = resize_linear(c, nw, nh, dtype)
        if quantize:
            r = np.rint(r)  # half to even
    return normalize(pad_center(r, S, left, top, pad, dtype), mean, std, to_rgb, dtype)


def extract_all(frames, frame_index, geoms, valids, S, **kw):
    F = frames.shape[0]
    return np.stack([extract(frames[min(max(int(f), 0), F - 1)], g, bool(v) and 0 <= int(f) < F,
                             S, **kw) for f, g, v in zip(frame_index, geoms, valids)])


# ------------------------------------------------------------------------------ PyTorch loop
def torch_patches(frames, frame_index, geom, valid, S, pad=128.0, mean=None, std=None,
                  to_rgb=False, quantize=True):
    """The per-object PyTorch version on ``frames``' device: frames [F, H, W, C] uint8 →
    [N, C, S, S] float32.  ``geom.tolist()`` is its host synchronisation."""
    import torch
    import torch.nn.functional as Fn
    F, H, W, C = frames.shape
    dev = frames.device
    mean = torch.tensor([0.0] * C if mean is None else list(mean), device=dev).view(C, 1, 1)
    std = torch.tensor([1.0] * C if std is None else list(std), device=dev).view(C, 1, 1)
    out = torch.full((len(geom), C, S, S), float(pad), device=dev)
    for i, (g, f, v) in enumerate(zip(geom.tolist(), frame_index.tolist(), valid.tolist())):
        if not v or not 0 <= f < F:
            continue
        x1, y1, x2, y2, nw, nh, left, top = g
        img = frames[f].permute(2, 0, 1).float()
        pl, pt, pr, pb = max(-x1, 0), max(-y1, 0), max(x2 - W + 1, 0), max(y2 - H + 1, 0)
        img = Fn.pad(img, (pl, pr, pt, pb), value=float(pad))
        img = img[:, y1 + pt:y2 + pt + 1, x1 + pl:x2 + pl + 1]
        img = Fn.interpolate(img[None], size=(nh, nw), mode="bilinear", align_corners=False)[0]
        out[i, :, top:top + nh, left:left + nw] = img.round() if quantize else img
    if to_rgb:
        out = out.flip(1)
    return (out - mean) / std
