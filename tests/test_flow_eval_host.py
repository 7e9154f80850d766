"""CPU: the flow-validation restatement (tests/flow_eval_restatement.py) against the reference's own
run (golden/golden_flow_eval.npz, golden/make_golden_flow_eval.py), the C layout of the two new
argument structs, and the argument errors of scflow_flow_gt / scflow_flow_epe and their wrappers —
all of which come before any launch, so none of this needs a GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scflow_amd import _lib, flow_eval, ops
from scflow_amd._lib import ScflowError
from tests import flow_eval_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_flow_eval.npz")
REL = 1e-9  # fp64 against fp64


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def scene():
    b = fr.scene_case("fixture")
    return b, fr.scene_gt_flow(b)


def bits(flow, inv=400.0):
    return ((flow[:, 0] == inv) & (flow[:, 1] == inv)).numpy()


def unpack(packed, shape):
    return np.unpackbits(packed)[: int(np.prod(shape))].reshape(shape).astype(bool)


def close(a, b, rel=REL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300))


def sums(f):
    return np.array([float(f.sum()), float(f.abs().sum())])


def test_fixture_is_the_batch_the_tests_regenerate(gold):
    assert list(gold["meta"]) == [fr.FIXTURE["batch"], fr.FIXTURE["size"], fr.FIXTURE["seed"]]
    assert 0.02 <= float(gold["removed"]) <= 0.5 and float(gold["near_share"]) <= 0.01
    assert int(gold["depth_rewritten"]) > 0


def test_gt_flow_restatement_equals_reference(gold, scene):
    _, flow = scene
    assert np.array_equal(bits(flow), unpack(gold["bits_flow"], bits(flow).shape))
    assert close(sums(flow), gold["sum_flow"])


@pytest.mark.parametrize("which", ["mask", "depth_reference", "face", "all_reference"])
def test_filter_restatement_equals_reference(gold, scene, which):
    b, flow = scene
    near = torch.zeros_like(flow[:, 0], dtype=torch.bool)
    src = flow
    if which == "mask":
        bad, near = fr.mask_filter(flow, b["gt_masks"])
    elif which == "depth_reference":
        src = fr.mark_invalid(flow)
        bad, near = fr.depth_filter(src, b["gt_depth"], b["depth"], combine="reference")
    elif which == "face":
        bad, near = fr.face_filter(flow, b["face_index"], b["gt_face_index"])
    else:  # one after another, each on the previous one's output, as the reference's callers would
        out = flow
        for f, args in ((fr.mask_filter, (b["gt_masks"],)),
                        (fr.depth_filter, (b["gt_depth"], b["depth"], 400.0, 0.2, "reference")),
                        (fr.face_filter, (b["face_index"], b["gt_face_index"]))):
            bad_k, near_k = f(out, *args)
            out, near = fr.apply_filter(out, bad_k), near | near_k
        # … which is what deciding everything from the unfiltered flow gives (the fused kernel)
        fused = (fr.mask_filter(flow, b["gt_masks"])[0] |
                 fr.depth_filter(flow, b["gt_depth"], b["depth"], combine="reference")[0] |
                 fr.face_filter(flow, b["face_index"], b["gt_face_index"])[0])
        assert torch.equal(bits_t(out), bits_t(fr.apply_filter(flow, fused)))
    if which != "all_reference":
        out = fr.apply_filter(src, bad)
    got, want = bits(out), unpack(gold[f"bits_{which}"], bits(out).shape)
    assert not np.any((got != want) & ~near.numpy())
    assert float(near.double().mean()) <= 0.01
    if np.array_equal(got, want):  # the face filter's reference run is float32 (its sampled map is)
        assert close(sums(out), gold[f"sum_{which}"], REL if which in ("mask", "depth_reference") else 1e-6)


def bits_t(flow, inv=400.0):
    return (flow[:, 0] == inv) & (flow[:, 1] == inv)


def test_depth_reference_mode_is_observable_and_or_mode_is_not_a_noop(gold, scene):
    b, flow = scene
    marked = fr.mark_invalid(flow)
    ref_bad, _ = fr.depth_filter(marked, b["gt_depth"], b["depth"], combine="reference")
    out = fr.apply_filter(marked, ref_bad)
    assert int((out != marked).any(1).sum()) == int(gold["depth_rewritten"]) > 0
    # on a freshly built GT flow the reference's & rewrites nothing; 'or' removes valid pixels
    fresh_ref, _ = fr.depth_filter(flow, b["gt_depth"], b["depth"], combine="reference")
    assert torch.equal(fr.apply_filter(flow, fresh_ref), flow)
    bad_or, near = fr.depth_filter(flow, b["gt_depth"], b["depth"], combine="or")
    cons = unpack(gold["bits_consistent"], tuple(bad_or.shape))
    want = bits(flow) | ~cons
    assert not np.any((bad_or.numpy() != want) & ~near.numpy())
    assert int((bad_or & ~bits_t(flow)).sum()) > 0


@pytest.mark.parametrize("tag", ["nomask", "mask"])
def test_cal_epe_restatement_equals_reference(gold, tag):
    tgt, pred, mask, _ = fr.epe_case("fixture")
    m = None if tag == "nomask" else mask
    tm = fr.cal_epe(tgt, pred, m, reduction="total_mean")
    want = gold[f"epe_total_mean_{tag}"]
    assert close(float(tm["mean"]), want[0])
    # the reference divides the integer counts by ``count + 1e-10``, a float32 tensor: its accuracies
    # are float32 quotients (one rounding, 6e-8 relative) even in its float64 run
    assert close([float(tm[k]) for k in ("1px", "3px", "5px")], want[1:], 1e-7)
    assert close(fr.cal_epe(tgt, pred, m, reduction="mean")["mean"].numpy(), gold[f"epe_mean_{tag}"])
    none = fr.cal_epe(tgt, pred, m, reduction="none").numpy()
    assert np.all(np.abs(none - gold[f"epe_none_{tag}"]) <= REL * np.maximum(gold[f"epe_none_{tag}"], 1.0))
    # 'mean': the accuracies are over the valid pixels (the documented deviation), so they are
    # consistent with 'total_mean' through the valid counts
    st = fr.epe_stats(tgt, pred, m)
    per = fr.cal_epe(tgt, pred, m, reduction="mean")
    for k, t in enumerate((1, 3, 5)):
        assert close(float((per[f"{t}px"] * st["count"]).sum() / st["count"].sum()), float(tm[f"{t}px"]), 1e-12)
    assert float(per["1px"].max()) <= 1.0


def test_occlusion_term_and_empty_sample():
    tgt, pred, mask, occ = fr.epe_case("rect")
    st = fr.epe_stats(tgt, pred, mask, occ_pred=occ)
    assert int(st["count"][1]) == 0 and float(st["err_sum"][1]) == 0.0  # sample 1 has no depth
    per = fr.cal_epe(tgt, pred, mask, reduction="mean")
    assert float(per["mean"][1]) == 0.0 and torch.isfinite(per["mean"]).all()
    # no valid pixel: every |0 − occ| term is occ itself
    assert close(float(st["occ_sum"][1]), float(occ[1].double().sum()), 1e-12)
    ev = fr.eval_epe_and_occ(pred, occ, tgt, None, noc_without_mask=True)
    assert float(ev["epe_noc_mean"]) == float(ev["epe_mean"]) and 0.0 < float(ev["occ"]) < 1.0


# ------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("pyname,cname", [("FlowGtArgs", "scflow_flow_gt_args"),
                                           ("FlowEpeArgs", "scflow_flow_epe_args")])
def test_struct_layout_matches_header(tmp_path, pyname, cname):
    """ctypes argument structs have the C compiler's size and field offsets (test_abi.py's way)."""
    S = getattr(_lib, pyname)
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f for f, _ in S._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scflow_hip.h"\nint main(){\n'
                    f'printf("%zu\\n", sizeof({cname}));\n' +
                    "".join(f'printf("%zu\\n", offsetof({cname}, {f}));\n' for f in fields) +
                    "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                           check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(S)
    for f, off in zip(fields, vals[1:]):
        assert getattr(S, f).offset == off, f


def _gt_args(**kw):
    """Arguments that pass every check but the one under test (the pointers are never read)."""
    a = _lib.FlowGtArgs()
    for f in ("depth", "K", "R_ref", "t_ref", "R_gt", "t_gt", "flow"):
        setattr(a, f, 64)
    a.n, a.h, a.w, a.invalid_num = 1, 8, 8, 400.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.scflow_flow_gt(None, None) == -1
    assert lib.scflow_flow_epe(None, None) == -1
    for bad in (dict(n=0), dict(h=0), dict(w=-1), dict(flow=None), dict(K=None), dict(flow_in=128),
                dict(depth_combine=2), dict(mask_dtype=2), dict(face_dtype=4), dict(face_index1=256),
                dict(depth=None), dict(flow_filtered=64)):
        assert lib.scflow_flow_gt(ctypes.byref(_gt_args(**bad)), None) == -1, bad
    only_flow_in = _gt_args(K=None, R_ref=None, t_ref=None, R_gt=None, t_gt=None, depth=None,
                            flow_in=128, depth1=512)
    assert lib.scflow_flow_gt(ctypes.byref(only_flow_in), None) == -1  # depth filter without depth0
    assert lib.scflow_flow_gt(ctypes.byref(_gt_args(h=1 << 15, w=1 << 15)), None) == -2
    e = _lib.FlowEpeArgs()
    e.flow_tgt, e.flow_pred, e.counts, e.sums, e.workspace = 64, 128, 256, 512, 1024
    e.n, e.h, e.w, e.workspace_bytes = 2, 20, 36, 1 << 20
    for bad in (dict(n=0), dict(flow_pred=None), dict(counts=None), dict(workspace=None),
                dict(workspace_bytes=8)):
        b = _lib.FlowEpeArgs.from_buffer_copy(e)
        for k, v in bad.items():
            setattr(b, k, v)
        assert lib.scflow_flow_epe(ctypes.byref(b), None) == -1, bad
    b = _lib.FlowEpeArgs.from_buffer_copy(e)
    b.workspace = 1028
    assert lib.scflow_flow_epe(ctypes.byref(b), None) == -3
    # 20·36 = 720 pixels → 3 workgroups per sample, 2 doubles + 4 ints each
    assert lib.scflow_flow_epe_workspace(2, 20, 36) == 2 * 3 * 32
    assert lib.scflow_flow_epe_workspace(1, 256, 256) == 64 * 32
    assert lib.scflow_flow_epe_workspace(0, 8, 8) == -1


def test_wrappers_raise_before_any_launch():
    flow = torch.zeros(2, 2, 8, 12)
    with pytest.raises(ValueError, match="contiguous"):
        ops.flow_gt(flow_in=flow.transpose(2, 3))
    with pytest.raises(ValueError, match="contiguous"):
        ops.flow_epe(flow, flow.transpose(2, 3))
    with pytest.raises(ValueError, match="not both"):
        ops.flow_gt(K=torch.eye(3)[None], flow_in=flow)
    with pytest.raises(ValueError, match="needs depth"):
        ops.flow_gt(depth=torch.zeros(2, 8, 12))
    with pytest.raises(ValueError, match="empty"):
        ops.flow_gt(flow_in=torch.zeros(0, 2, 8, 12))
    with pytest.raises(ValueError, match="empty"):
        ops.flow_epe(torch.zeros(0, 2, 8, 12), torch.zeros(0, 2, 8, 12))
    with pytest.raises(ScflowError, match="no CPU fallback"):
        ops.flow_gt(flow_in=flow)  # a CPU tensor: there is no CPU path
    with pytest.raises(ScflowError, match="no CPU fallback"):
        ops.flow_epe(flow, flow)
    with pytest.raises(NotImplementedError):
        flow_eval.filter_flow_by_mask(flow, torch.ones(2, 8, 12), mode="nearest")
    with pytest.raises(ValueError, match="reduction"):
        flow_eval.cal_epe(flow, flow, None, reduction="sum")
    assert hasattr(torch.ops.scflow, "flow_gt") and hasattr(torch.ops.scflow, "flow_epe")


def test_fake_implementations_give_the_shapes():
    m = dict(device="meta")
    flow, filt = torch.ops.scflow.flow_gt(torch.empty(3, 20, 36, **m), torch.empty(3, 3, 3, **m),
                                          torch.empty(3, 3, 3, **m), torch.empty(3, 3, **m),
                                          torch.empty(3, 3, 3, **m), torch.empty(3, 3, **m), None, 400.0,
                                          None, None, 0.2, "or", None, None)
    assert flow.shape == filt.shape == (3, 2, 20, 36)
    c, s, e = torch.ops.scflow.flow_epe(torch.empty(3, 2, 20, 36, **m), torch.empty(3, 2, 20, 36, **m),
                                        None, 400.0, [1.0, 3.0, 5.0], None, True, True)
    assert c.shape == (3, 4) and c.dtype == torch.int32 and s.shape == (3, 2) and s.dtype == torch.float64
    assert e.shape == (3, 20, 36)
