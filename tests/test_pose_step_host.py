"""CPU: the pose step's argument refusals, through every entry that can express the call.

``scflow_pose_step``, ``_part``, ``_heads`` and ``_masked`` are fills of ``scflow_pose_step_args``
in front of one launcher, ``scflow_pose_step_call`` is that launcher.  A refused call returns
before any launch, so it needs no device; accepted calls are not made here (they would launch).

Each case is ``BASE`` (a call every entry accepts) with a few fields replaced, and the status the
entries returned before they shared a launcher: the line of the check in that revision's
``csrc/pose.hip`` (the four entry bodies, lines 243-356) or ``csrc/pose_dev.h`` (the positional
``pose_step_args``, lines 412-446) stands beside it.  All of them are SCFLOW_EINVAL (-1) but the
alignment check, SCFLOW_EALIGN (-3), which came after every other check of ``pose_step_args``
and before the entries' empty-``parts`` refusal.
"""
import ctypes

import pytest

from scflow_amd import _lib

EINVAL, EALIGN = -1, -3
QUAT = 16  # SCFLOW_POSE_QUAT_XYZW

# fake device pointers: non-null, 16-byte aligned, all different (never dereferenced)
_NAMES = ("x", "xbias", "Wr", "br", "Wt", "bt", "label", "drot", "dt", "R_src", "t_src", "K", "points",
          "R_dst", "t_dst", "flow", "lr", "delta", "mask", "flow_up", "mask_up", "lr_next", "hx_next",
          "mask_next", "lrm_next")
P = {name: 0x10000 + 0x100 * i for i, name in enumerate(_NAMES)}

# scflow_pose_step's call: n = 3, 128² from a 16² map, every output wanted
BASE = dict(x=None, xsplit=0, xbias=None, k=0, Wr=None, br=None, rch=0, Wt=None, bt=None, label=None,
            num_class=0,
            drot=P["drot"], dt=P["dt"], R_src=P["R_src"], t_src=P["t_src"], K=P["K"],
            points=P["points"], R_dst=P["R_dst"], t_dst=P["t_dst"], flow=P["flow"],
            n=3, H=128, W=128, weight=10.0, depth_transform=0, invalid_num=400.0,
            lr=P["lr"], delta=P["delta"], mask=P["mask"], flow_up=P["flow_up"], mask_up=P["mask_up"],
            h=16, w=16, up_scale=8.0, down_scale=0.125,
            lr_next=P["lr_next"], s_next=2, hx_next=P["hx_next"], s_hx=6,
            mask_next=None, lrm_next=None, s_lrm=0, parts=3)
HEADS = dict(x=P["x"], xsplit=4, xbias=P["xbias"], k=256, Wr=P["Wr"], br=P["br"], rch=6, Wt=P["Wt"],
             bt=P["bt"], label=P["label"], num_class=21)
MASKED = dict(mask_next=P["mask_next"], lrm_next=P["lrm_next"], s_lrm=2)
NO_NEXT = dict(lr_next=None, s_next=0, hx_next=None, s_hx=0)
GIVEN = dict(drot=None, dt=None, R_dst=None, t_dst=None, parts=1, **NO_NEXT)  # ops.pose_step_given's

# the positional exports' parameter orders (include/scflow_hip.h)
_HEAD_ORDER = ["x", "xsplit", "xbias", "k", "Wr", "br", "rch", "Wt", "bt", "label", "num_class"]
_STEP_ORDER = ["drot", "dt", "R_src", "t_src", "K", "points", "R_dst", "t_dst", "flow", "n", "H", "W",
               "weight", "depth_transform", "invalid_num", "lr", "delta", "mask", "flow_up", "mask_up",
               "lr_next", "s_next", "hx_next", "s_hx"]
_TAIL_ORDER = ["h", "w", "up_scale", "down_scale"]
ORDERS = {
    "scflow_pose_step": _STEP_ORDER + _TAIL_ORDER,
    "scflow_pose_step_part": _STEP_ORDER + _TAIL_ORDER + ["parts"],
    "scflow_pose_step_heads": _HEAD_ORDER + _STEP_ORDER + _TAIL_ORDER + ["parts"],
    "scflow_pose_step_masked": (_HEAD_ORDER + _STEP_ORDER + ["mask_next", "lrm_next", "s_lrm"] +
                                _TAIL_ORDER + ["parts"]),
}


def test_orders_cover_the_struct():
    fields = [f for f, _ in _lib.PoseStepArgs._fields_]
    assert sorted(ORDERS["scflow_pose_step_masked"]) == sorted(fields) == sorted(BASE)
    for name, order in ORDERS.items():
        assert len(order) + 1 == len(_lib.SIGNATURES[name][1]), name  # + the stream


def expressible(entry, c):
    """Whether the positional ``entry`` has a parameter for everything case ``c`` sets, and the
    case is not one that this entry alone refuses (those: test_entry_specific_refusals)."""
    heads_off = all(not c[f] for f in _HEAD_ORDER)
    masked_off = all(not c[f] for f in ("mask_next", "lrm_next", "s_lrm"))
    if entry == "scflow_pose_step":
        return heads_off and masked_off and c["parts"] == 3 and c["drot"] is not None
    if entry == "scflow_pose_step_part":
        return heads_off and masked_off
    if entry == "scflow_pose_step_heads":
        return masked_off and c["x"] is not None
    return c["drot"] is not None  # scflow_pose_step_masked


def statuses(c):
    """{entry: status} of case ``c`` through scflow_pose_step_call and every expressible export."""
    lib = _lib.load()
    a = _lib.PoseStepArgs()
    for f, v in c.items():
        setattr(a, f, v)
    out = {"scflow_pose_step_call": lib.scflow_pose_step_call(ctypes.byref(a), None)}
    for entry, order in ORDERS.items():
        if expressible(entry, c):
            out[entry] = getattr(lib, entry)(*[c[f] for f in order], None)
    return out


# (what is wrong, fields replaced in BASE, status, where the parent checked it)
REFUSED = [
    ("R_src missing", dict(R_src=None), EINVAL, "pose_dev.h:421"),
    ("t_src missing", dict(t_src=None), EINVAL, "pose_dev.h:421"),
    ("K missing", dict(K=None), EINVAL, "pose_dev.h:421"),
    ("points missing", dict(points=None), EINVAL, "pose_dev.h:421"),
    ("flow missing", dict(flow=None), EINVAL, "pose_dev.h:421"),
    ("a delta without dt", dict(dt=None), EINVAL, "pose_dev.h:421"),
    ("a delta without R_dst", dict(R_dst=None), EINVAL, "pose_dev.h:421"),
    ("a delta without t_dst", dict(t_dst=None), EINVAL, "pose_dev.h:421"),
    ("n = 0", dict(n=0), EINVAL, "pose_dev.h:422"),
    ("H = 0", dict(H=0), EINVAL, "pose_dev.h:422"),
    ("W < 0", dict(W=-1), EINVAL, "pose_dev.h:422"),
    ("depth_transform bit 1", dict(depth_transform=2), EINVAL, "pose_dev.h:422"),
    ("depth_transform bit 5", dict(depth_transform=QUAT | 32), EINVAL, "pose_dev.h:422"),
    ("outputs at h = 0", dict(h=0), EINVAL, "pose_dev.h:425"),
    ("lr_next at w = 0", dict(w=0, flow_up=None), EINVAL, "pose_dev.h:425"),
    ("flow_up without lr", dict(lr=None), EINVAL, "pose_dev.h:426"),
    ("lr_next with s_next 1", dict(s_next=1), EINVAL, "pose_dev.h:427"),
    ("lr_next aliasing lr", dict(lr_next=P["lr"]), EINVAL, "pose_dev.h:427"),
    ("hx_next with s_hx 1", dict(s_hx=1), EINVAL, "pose_dev.h:427"),
    ("points misaligned", dict(points=P["points"] + 4), EALIGN, "pose_dev.h:428"),
    ("points misaligned, ↓8 part alone", dict(points=P["points"] + 8, parts=2), EALIGN, "pose_dev.h:428"),
    ("points misaligned, full part alone", dict(points=P["points"] + 4, parts=1), EALIGN, "pose_dev.h:428"),
    # (the alignment check ran before the entries looked at an empty launch)
    ("points misaligned before parts = 2 without lr_next", dict(points=P["points"] + 4, parts=2, **NO_NEXT),
     EALIGN, "pose_dev.h:428 before pose.hip:279"),
    ("parts = 0", dict(parts=0), EINVAL, "pose.hip:270,296,333"),
    ("parts = 4", dict(parts=4), EINVAL, "pose.hip:270,296,333"),
    ("parts < 0", dict(parts=-1), EINVAL, "pose.hip:270,296,333"),
    ("parts = 2 without lr_next", dict(parts=2, **NO_NEXT), EINVAL, "pose.hip:279,308,347"),
    ("given pose with parts = 2", dict(GIVEN, parts=2), EINVAL, "pose.hip:270"),
    ("given pose with parts = 3", dict(GIVEN, parts=3), EINVAL, "pose.hip:270"),
    ("given pose with lr_next", dict(GIVEN, lr_next=P["lr_next"], s_next=2), EINVAL, "pose_dev.h:424"),
    ("given pose without R_src", dict(GIVEN, R_src=None), EINVAL, "pose_dev.h:421"),
    # the heads block
    ("heads: xsplit 0", dict(HEADS, xsplit=0), EINVAL, "pose.hip:295,334"),
    ("heads: xbias missing", dict(HEADS, xbias=None), EINVAL, "pose.hip:295,334"),
    ("heads: k 0", dict(HEADS, k=0), EINVAL, "pose.hip:295,334"),
    ("heads: Wr missing", dict(HEADS, Wr=None), EINVAL, "pose.hip:295,334"),
    ("heads: br missing", dict(HEADS, br=None), EINVAL, "pose.hip:295,334"),
    ("heads: Wt missing", dict(HEADS, Wt=None), EINVAL, "pose.hip:295,334"),
    ("heads: bt missing", dict(HEADS, bt=None), EINVAL, "pose.hip:295,334"),
    ("heads: label missing", dict(HEADS, label=None), EINVAL, "pose.hip:295,334"),
    ("heads: num_class 0", dict(HEADS, num_class=0), EINVAL, "pose.hip:296,335"),
    ("heads: dt (an output) missing", dict(HEADS, dt=None), EINVAL, "pose.hip:296,335"),
    ("heads: rch 4 for ortho6d", dict(HEADS, rch=4), EINVAL, "pose.hip:296,335"),
    ("heads: rch 6 for a quaternion", dict(HEADS, depth_transform=QUAT | 1), EINVAL, "pose.hip:296,335"),
    ("heads: rch 5", dict(HEADS, rch=5), EINVAL, "pose.hip:296,335"),
    ("heads: parts = 4", dict(HEADS, parts=4), EINVAL, "pose.hip:296,333"),
    ("heads: parts = 2 without lr_next", dict(HEADS, parts=2, **NO_NEXT), EINVAL, "pose.hip:308,347"),
    ("heads: R_src missing", dict(HEADS, R_src=None), EINVAL, "pose_dev.h:421"),
    ("heads: points misaligned", dict(HEADS, points=P["points"] + 4), EALIGN, "pose_dev.h:428"),
    # the masked tail
    ("mask_next without lr_next", dict(NO_NEXT, mask_next=P["mask_next"], parts=1), EINVAL, "pose.hip:337"),
    ("lrm_next without lr_next", dict(NO_NEXT, lrm_next=P["lrm_next"], s_lrm=2, parts=1), EINVAL,
     "pose.hip:337"),
    ("lrm_next aliasing lr", dict(MASKED, lrm_next=P["lr"]), EINVAL, "pose.hip:338"),
    ("lrm_next aliasing lr_next", dict(MASKED, lrm_next=P["lr_next"]), EINVAL, "pose.hip:338"),
    ("lrm_next with s_lrm 1", dict(MASKED, s_lrm=1), EINVAL, "pose.hip:338"),
    ("lrm_next with s_lrm 1, no mask", dict(MASKED, mask_next=None, s_lrm=1), EINVAL, "pose.hip:338"),
    ("masked: points misaligned", dict(MASKED, points=P["points"] + 4), EALIGN, "pose_dev.h:428"),
    ("masked + heads: label missing", dict(HEADS, **MASKED, label=None), EINVAL, "pose.hip:334"),
    ("masked + heads: lrm_next aliasing lr", dict(HEADS, **dict(MASKED, lrm_next=P["lr"])), EINVAL,
     "pose.hip:338"),
]


@pytest.mark.parametrize("what,change,status,where", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_before_any_launch(what, change, status, where):
    got = statuses(dict(BASE, **change))
    assert got == {entry: status for entry in got}, (what, where, got)


def test_every_entry_is_reached_by_the_table():
    reached = set()
    for _, change, _, _ in REFUSED:
        c = dict(BASE, **change)
        reached |= {e for e in ORDERS if expressible(e, c)}
    assert reached == set(ORDERS)


def test_entry_specific_refusals():
    """What only one entry refuses stays in that entry.  The given-pose form (drot NULL, parts 1)
    is scflow_pose_step_part's and the struct entry's: with misaligned points they get as far as
    the alignment check (every EINVAL check passed), while scflow_pose_step (pose.hip:251) and
    scflow_pose_step_masked (pose.hip:333) refuse the form itself.  scflow_pose_step_heads
    refuses a call without x (pose.hip:295) that scflow_pose_step_masked reads as _part's."""
    lib = _lib.load()
    c = dict(BASE, **GIVEN, points=P["points"] + 4)
    got = statuses(c)
    assert got == {"scflow_pose_step_call": EALIGN, "scflow_pose_step_part": EALIGN}
    masked = lib.scflow_pose_step_masked(*[c[f] for f in ORDERS["scflow_pose_step_masked"]], None)
    assert masked == EINVAL
    c3 = dict(c, parts=3)  # (scflow_pose_step has no parts parameter)
    assert lib.scflow_pose_step(*[c3[f] for f in ORDERS["scflow_pose_step"]], None) == EINVAL
    # x NULL through the heads entry, the rest as BASE with misaligned points: _masked and _part
    # reach the alignment check
    c = dict(BASE, points=P["points"] + 4)
    assert lib.scflow_pose_step_heads(*[c[f] for f in ORDERS["scflow_pose_step_heads"]], None) == EINVAL
    assert statuses(c)["scflow_pose_step_masked"] == EALIGN
    assert lib.scflow_pose_step_call(None, None) == EINVAL
