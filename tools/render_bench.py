"""Timing of the renderer: vertex-coloured, UV-textured and mixed batches
through `Renderer.forward`, on the device, alternating in one process.

usage: python tools/render_bench.py [--batch 32] [--size 256] [--tex 1024] [--rounds 9] [--steps 50]
                                    [--vertex-only] [--json out.json]

The scene is `bench.py`'s `end_to_end.render` leg: `batch` images at `size`², the 21 stand-in
objects as 24×48 ellipsoids (2208 faces), `synthetic.make_scene` poses, separate lights.  Timed,
each window between two device events around `steps` calls of `Renderer.forward` (host packing
included, as in `bench.py`), after a warm-up of every configuration:

* `vertex`:   every mesh vertex-coloured — `scflow_render`, the path of the YCB-V configs;
* `textured`: every mesh UV-textured with its own `tex`² map (`synthetic.textured_ellipsoid_mesh`)
  — `scflow_render_textured`;
* `mixed`:    the meshes of the odd labels textured, the others vertex-coloured, in one batch.

`--vertex-only` times `vertex` alone and uses nothing a checkout without UV textures lacks, so the
same file measures such a checkout.  Prints the medians, the texel traffic of the textured batch —
covered pixels × 4 taps × 4 B requested, and the distinct texels those taps touch × 4 B — and one
JSON line.  No threshold: DESIGN.md §21 compares `vertex` across checkouts.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def texel_traffic(r, out, labels):
    """(covered pixels of textured images, distinct texels their four taps touch) of a render."""
    p2f = out["fragments"].pix_to_face[..., 0]
    bary = out["fragments"].bary_coords[..., 0, :]
    covered = distinct = off = 0
    for i, lab in enumerate(labels):
        nf = r.meshes[lab][1].shape[0]
        if lab in r.textures:
            uv, fuv, img = r.textures[lab]
            h, w = int(img.shape[0]), int(img.shape[1])
            hit = p2f[i] >= 0
            f = (p2f[i][hit] - off).long()
            puv = (bary[i][hit][:, :, None] * uv[fuv[f].long()]).sum(1)
            x = (puv[:, 0] * (w - 1)).clamp(0, w - 1)
            y = ((1 - puv[:, 1]) * (h - 1)).clamp(0, h - 1)
            x0, y0 = x.floor().long(), y.floor().long()
            x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
            taps = torch.cat([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1])
            covered += int(hit.sum())
            distinct += int(torch.unique(taps).numel())
        off += nf
    return covered, distinct


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--tex", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--vertex-only", action="store_true",
                    help="time the vertex-coloured batch alone (also on a checkout without UV textures)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU: a CPU run says nothing about these timings")
    from scflow_amd import synthetic
    from scflow_amd.renderer import Renderer
    dev = torch.device("cuda")
    sc = synthetic.make_scene(a.batch, a.size, seed=1000)
    args = tuple(torch.from_numpy(sc[k]).to(dev) for k in ("ref_rotation", "ref_translation",
                                                           "internel_k", "labels"))
    labels = sc["labels"].tolist()
    semi = {lab: [x * synthetic.YCBV_DIAMETERS[lab] for x in synthetic.ELLIPSOID_AXES] for lab in range(21)}
    plain = {lab: synthetic.ellipsoid_mesh(semi[lab], 24, 48) for lab in range(21)}  # 2208 faces
    kinds = {"vertex": plain}
    if not a.vertex_only:
        tex = {lab: synthetic.textured_ellipsoid_mesh(semi[lab], 24, 48, (a.tex, a.tex), seed=lab)
               for lab in range(21)}
        kinds["textured"] = tex
        kinds["mixed"] = {lab: tex[lab] if lab % 2 else plain[lab] for lab in range(21)}
    rs = {k: Renderer(image_size=(a.size, a.size), soft_blending=False, render_mask=False,
                      seperate_lights=True, meshes=m).to(dev) for k, m in kinds.items()}
    outs = {}
    for k, r in rs.items():  # warm every configuration (code objects, allocator, texel store)
        for _ in range(3):
            outs[k] = r(*args)
    torch.cuda.synchronize()
    times = {k: [] for k in rs}
    for _ in range(a.rounds):
        for k, r in rs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                r(*args)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.steps)
    v = outs["vertex"]  # a digest of the vertex-coloured render: equal across checkouts that agree bit for bit
    digest = hashlib.sha256(b"".join(x.contiguous().cpu().numpy().tobytes() for x in (
        v["images"], v["fragments"].zbuf, v["fragments"].bary_coords, v["fragments"].pix_to_face))).hexdigest()
    res = dict(batch=a.batch, size=a.size, faces=int(plain[0][1].shape[0]), rounds=a.rounds, steps=a.steps,
               covered=int((v["fragments"].pix_to_face >= 0).sum()), vertex_sha256=digest[:16])
    for k, v in times.items():
        res[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        print(f"{k}: median {res[k]['median_ms']:.4f} ms/batch (min {min(v):.4f}, max {max(v):.4f})")
    if not a.vertex_only:
        for k in ("textured", "mixed"):
            cov, distinct = texel_traffic(rs[k], outs[k], labels)
            res[k].update(textured_images=sum(lab in rs[k].textures for lab in labels), covered=cov,
                          tap_bytes=cov * 16, distinct_texel_bytes=distinct * 4,
                          store_bytes=int(rs[k].texture_store()["texels"].numel()))
        same = torch.equal(outs["vertex"]["fragments"].zbuf, outs["textured"]["fragments"].zbuf)
        res.update(tex=a.tex, same_zbuf=bool(same),
                   textured_over_vertex=res["textured"]["median_ms"] / res["vertex"]["median_ms"])
        t = res["textured"]
        print(f"N={a.batch} images at {a.size}², {res['faces']}-face meshes, {a.tex}² maps: textured / "
              f"vertex = {res['textured_over_vertex']:.3f}×; the textured batch covers {t['covered']} "
              f"pixels, its taps request {t['tap_bytes'] / 1e6:.2f} MB and touch "
              f"{t['distinct_texel_bytes'] / 1e6:.2f} MB of distinct texels of a {t['store_bytes'] / 1e6:.1f} MB "
              f"store; zbuf {'equal' if same else 'DIFFERS'} bit for bit")
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
