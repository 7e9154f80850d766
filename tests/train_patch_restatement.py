"""NumPy restatement of the training-patch contract (include/scflow_hip.h
scflow_train_draw / scflow_patch_extract_aug): the counter-based generator, the draws and each
colour stage, stage by stage on the crop array as the reference's pipeline runs them; geometry and
resize come from tests/patch_restatement.py.

``dtype=np.float32`` performs every floating-point operation in fp32, one rounding per operation
in the contract's order; ``dtype=np.float64`` is the same definition in fp64.  The integer parts
(Philox, BGR → HSV, the blur) have one form.  NumPy's fp32 log / cos / sin are not the device's, so
normals restated in fp32 are close to the device's, not equal; everything that does not pass
through them is.
"""
import numpy as np

from tests import patch_restatement as pr

RNG_CROP, RNG_COLOUR, RNG_NOISE, RNG_JITTER = 0, 1, 2, 16
AUG_HSV, AUG_NOISE, AUG_BLUR = 1, 2, 4
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)

CFG = dict(angle_mean=0.0, angle_std=15.0, x_mean=0.0, y_mean=0.0, z_mean=0.0, x_std=15.0,
           y_std=15.0, z_std=50.0, angle_limit=45.0, translation_limit=200.0, add_limit=1.0,
           ratio_lo=1.0, ratio_hi=1.25, h_ratio=0.2, s_ratio=0.5, v_ratio=0.5, noise_ratio=0.1,
           max_kernel_size=5, p_hsv=1.0, p_noise=1.0, p_blur=1.0)


# ------------------------------------------------------------------------------ generator
def philox4x32(counter, key):
    """Philox4x32-10: counter [..., 4], key [2] (or [..., 2]) of uint32 → [..., 4] uint32."""
    c = [np.asarray(counter)[..., j].astype(np.uint64) for j in range(4)]
    k = [np.asarray(key)[..., j].astype(np.uint64) for j in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return np.stack(c, -1).astype(np.uint32)


def words(index, obj, stream, seed, step):
    """The four words of counter (index, object, stream, step) under ``seed``; ``index`` may be an
    array."""
    index = np.asarray(index, np.uint64)
    ctr = np.empty(index.shape + (4,), np.uint64)
    ctr[..., 0] = index
    ctr[..., 1] = obj
    ctr[..., 2] = stream | ((step >> 32) << 8)
    ctr[..., 3] = step & 0xFFFFFFFF
    return philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def u01(w, dtype=np.float32):
    return (w >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)


def u01_open(w, dtype=np.float32):
    """((w >> 8) + 0.5)·2^-24: in fp32 the sum is rounded to 24 bits."""
    return ((w >> np.uint32(8)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)


def normal3(w, dtype=np.float32):
    """Words [..., 4] → three Box–Muller normals [..., 3]: (w0, w1) → cos, sin; (w2, w3) → cos."""
    two_pi = dtype(np.float32(2 * np.pi)) if dtype is np.float32 else dtype(2 * np.pi)
    r0 = np.sqrt(dtype(-2) * np.log(u01_open(w[..., 0], dtype)))
    r1 = np.sqrt(dtype(-2) * np.log(u01_open(w[..., 2], dtype)))
    a0, a1 = two_pi * u01(w[..., 1], dtype), two_pi * u01(w[..., 3], dtype)
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], -1).astype(dtype)


# ------------------------------------------------------------------------------ draw
def euler_zyx(a, b, c):
    """ΔR = Rx(c)·Ry(b)·Rz(a), angles in degrees: scipy's from_euler('zyx', (a, b, c))."""
    a, b, c = np.deg2rad([a, b, c])
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    return Rx @ Ry @ Rz


def aug_row(obj, seed, step, cfg):
    """(ratio, aug row [8]) of an object in fp32, operation by operation."""
    f = np.float32
    lo, hi = f(cfg["ratio_lo"]), f(cfg["ratio_hi"])
    ratio = f(lo + f(u01(words(0, obj, RNG_CROP, seed, step)[0]) * f(hi - lo)))
    q0, q1 = (u01(words(i, obj, RNG_COLOUR, seed, step)) for i in (0, 1))
    row = np.zeros(8, f)
    for j, key in enumerate(("h_ratio", "s_ratio", "v_ratio")):
        row[j] = f(f(1) + f(f(f(2) * q0[j]) - f(1)) * f(cfg[key]))
    row[3] = f(q0[3] * f(cfg["noise_ratio"]))
    nk = (int(cfg["max_kernel_size"]) + 1) // 2
    row[4] = 2 * min(int(f(q1[0] * f(nk))), nk - 1) + 1
    row[5] = sum((1 << j) for j, key in enumerate(("p_hsv", "p_noise", "p_blur"))
                 if q1[1 + j] <= f(cfg[key]))
    return ratio, row


def draw(points, diameter, R_gt, t_gt, obj, seed, step, cfg, max_tries=32):
    """One object's jitter in fp64 from the same words: dict(R, t, add, rot, trans, ok, tries,
    margins) — ``margins``: the relative distance of every compared quantity to its limit, over
    all tries made."""
    R_gt, t_gt = np.asarray(R_gt, np.float64), np.asarray(t_gt, np.float64)
    X = np.asarray(points, np.float64)
    margins = []

    def over(value, limit):
        if limit < 0:
            return False
        margins.append(abs(value - limit) / max(limit, 1e-30))
        return value > limit

    for k in range(max_tries):
        z = normal3(words(0, obj, RNG_JITTER + k, seed, step), np.float64)
        ang = cfg["angle_mean"] + cfg["angle_std"] * z
        R = euler_zyx(*ang) @ R_gt
        rot = np.degrees(np.arccos(np.clip((np.trace(R @ R_gt.T) - 1) / 2, -1, 1)))
        if over(rot, cfg["angle_limit"]):
            continue
        z = normal3(words(1, obj, RNG_JITTER + k, seed, step), np.float64)
        dt = np.array([cfg["x_mean"], cfg["y_mean"], cfg["z_mean"]]) + \
            np.array([cfg["x_std"], cfg["y_std"], cfg["z_std"]]) * z
        trans = np.linalg.norm(dt)
        if over(trans, cfg["translation_limit"]):
            continue
        add = 0.0
        if len(X) and diameter > 0:
            add = np.linalg.norm((X @ R_gt.T + t_gt) - (X @ R.T + t_gt + dt), axis=1).mean() / diameter
            if over(add, cfg["add_limit"]):
                continue
        return dict(R=R, t=t_gt + dt, add=add, rot=rot, trans=trans, ok=1, tries=k + 1,
                    margins=margins)
    return dict(R=R_gt, t=t_gt, add=0.0, rot=0.0, trans=0.0, ok=0, tries=max_tries, margins=margins)


# ------------------------------------------------------------------------------ the stages
def bgr_to_hsv(img):
    """cv2's 8-bit COLOR_BGR2HSV in integers: [..., 3] uint8 → (h, s, v) int arrays."""
    b, g, r = (img[..., j].astype(np.int64) for j in range(3))
    v = np.maximum(b, np.maximum(g, r))
    d = v - np.minimum(b, np.minimum(g, r))
    vs, ds = np.maximum(v, 1), np.maximum(d, 1)
    sdiv = np.where(v > 0, (2 * (255 << 12) + vs) // (2 * vs), 0)   # round((255 << 12) / v)
    hdiv = np.where(d > 0, (2 * ((180 << 12) // 6) + ds) // (2 * ds), 0)  # round((180 << 12) / 6d)
    s = (d * sdiv + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * hdiv + 2048) >> 12  # floor
    return h + np.where(h < 0, 180, 0), s, v


def hsv_to_bgr(h, s, v, dtype=np.float32):
    """cv2's 8-bit COLOR_HSV2BGR through fp: integer h, s, v arrays → [..., 3] uint8."""
    f = dtype
    hh = h.astype(f) * f(f(6) / f(180))
    ss, vv = s.astype(f) * f(f(1) / f(255)), v.astype(f) * f(f(1) / f(255))
    fl = np.floor(hh)
    fr = (hh - fl).astype(f)
    sector = np.minimum(fl.astype(np.int64), 5)
    one = f(1)
    tab = np.stack([vv, vv * (one - ss), vv * (one - ss * fr), vv * (one - ss * (one - fr))], -1)
    sel = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]
    out = np.take_along_axis(tab, sel, -1)
    out = np.where((s == 0)[..., None], vv[..., None], out).astype(f)
    return np.clip(np.rint(out * f(255)), 0, 255).astype(np.uint8)


def hsv_stage(img, a, b, c, dtype=np.float32):
    f = dtype
    h, s, v = bgr_to_hsv(img)
    q = []
    for x, gain, top in ((h, a, 179), (s, b, 255), (v, c, 255)):
        y = x.astype(f) * f(np.float32(gain))
        if np.float32(gain) >= 1:
            y = np.minimum(y, f(top))
        q.append(np.clip(y, 0, top).astype(np.int64))  # truncation
    return hsv_to_bgr(*q, dtype=dtype)


def noise_values(img, sigma, obj, seed, step, dtype=np.float32):
    """x + (z·sigma)·255 before the clip: [ch, cw, 3] in ``dtype``; z keyed by y·cw + x."""
    ch, cw, _ = img.shape
    z = normal3(words(np.arange(ch * cw), obj, RNG_NOISE, seed, step), dtype).reshape(ch, cw, 3)
    return img.astype(dtype) + (z * dtype(np.float32(sigma))) * dtype(255)


def noise_stage(img, sigma, obj, seed, step, dtype=np.float32):
    return np.clip(noise_values(img, sigma, obj, seed, step, dtype), 0, 255).astype(np.uint8)


def fold101(p, n):
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p > n - 1, period - p, p)


def blur_stage(img, k):
    """cv2.blur(img, (k, k)) with BORDER_REFLECT_101: (2·Σ + k²) div (2·k²)."""
    if k == 1:
        return img
    ch, cw, _ = img.shape
    h = k // 2
    ys, xs = fold101(np.arange(-h, ch + h), ch), fold101(np.arange(-h, cw + h), cw)
    big = img[ys][:, xs].astype(np.int64)
    total = sum(big[dy:dy + ch, dx:dx + cw] for dy in range(k) for dx in range(k))
    return ((2 * total + k * k) // (2 * k * k)).astype(np.uint8)


def augment(crop, row, obj, seed, step, dtype=np.float32):
    """The three stages on a uint8 crop [ch, cw, 3] under an aug row."""
    mask = int(row[5]) if 0 <= row[5] < 8 else 0
    if mask & AUG_HSV:
        crop = hsv_stage(crop, row[0], row[1], row[2], dtype)
    if mask & AUG_NOISE:
        crop = noise_stage(crop, row[3], obj, seed, step, dtype)
    if mask & AUG_BLUR and row[4] in (3, 5):
        crop = blur_stage(crop, int(row[4]))
    return crop


def finish(crop, geom, S, pad=128, mean=None, std=None, to_rgb=False, quantize=True,
           dtype=np.float32):
    """Resize, quantise, pad and normalise an (augmented) uint8 crop: [3, S, S]."""
    mean = [0.0] * 3 if mean is None else mean
    std = [1.0] * 3 if std is None else std
    nw, nh, left, top = (int(v) for v in geom[4:])
    r = pr.resize_linear(crop, nw, nh, dtype)
    if quantize:
        r = np.rint(r)
    return pr.normalize(pr.pad_center(r, S, left, top, dtype(pad), dtype), mean, std, to_rgb, dtype)


def extract_aug(frame, geom, row, obj, S, seed, step, dtype=np.float32, pad=128, **kw):
    """One valid object's augmented patch [3, S, S] of ``frame`` [H, W, 3] uint8."""
    x1, y1, x2, y2 = (int(v) for v in geom[:4])
    crop = pr.crop(frame, x1, y1, x2, y2, pad, np.uint8)
    return finish(augment(crop, row, obj, seed, step, dtype), geom, S, pad=pad, dtype=dtype, **kw)
