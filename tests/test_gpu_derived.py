"""GPU: weight-derived forms (``scflow_amd/derived.py``) follow the weights at every site that
keeps one — the encoders' packings and eval-BatchNorm affine, the pose head's per-layer packings
and FC1 permutation, ``ConvRunner``'s form per launch shape.  fp32 throughout; a module whose
weights moved must compute exactly what a freshly built module with those weights computes."""
import ctypes

import pytest
import torch

from scflow_amd import synthetic

pytestmark = pytest.mark.gpu


def _encoder(norm, seed=11):
    from scflow_amd import MODELS
    enc = MODELS.build(dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
                            norm_cfg=dict(type=norm)))
    synthetic.fill_module_(enc, seed)
    return enc.eval().cuda()


def _fresh_like(enc, norm):
    fresh = _encoder(norm, seed=99)
    fresh.load_state_dict(enc.state_dict())
    return fresh.eval()


def _image(n, size=128, seed=5):
    return torch.rand(n, 3, size, size, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("norm", ["IN", "BN"])
def test_encoder_forms_follow_in_place_updates(norm):
    """128² image, the smallest the encoder runs (at 64² the last stage's 8×8 stride-1 maps are
    outside ``scflow_enc_conv``'s row tiles: SCFLOW_EUNSUPPORTED): the stem, Winograd stages at
    widths 64 and 32, ``enc_conv`` for the stride-2, 1×1 and 16-wide convs."""
    enc, x = _encoder(norm), _image(1)
    first = enc.forward_cl(x).clone()
    with torch.no_grad():
        for p in enc.parameters():
            p.mul_(1.01)
        for name, b in enc.named_buffers():
            if name.endswith(("running_mean", "running_var")):
                b.mul_(1.01)
    second = enc.forward_cl(x)
    want = _fresh_like(enc, norm).forward_cl(x)
    assert torch.equal(second, want)
    assert not torch.equal(second, first)


def test_eval_affine_follows_the_training_batchnorm():
    """eval → a train-mode forward under no_grad (the HIP BatchNorm writes the running
    statistics through raw pointers; γ/β untouched) → eval: the last eval forward uses the new
    statistics."""
    from scflow_amd.train.model import encoder_train
    enc, x = _encoder("BN"), _image(2)
    first = enc.forward_cl(x).clone()
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    enc.train()
    with torch.no_grad():
        encoder_train(enc, x.permute(0, 2, 3, 1).contiguous())
    enc.eval()
    torch.cuda.synchronize()
    moved = [k for k, v in enc.state_dict().items() if not torch.equal(v, before[k])]
    assert moved and all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in moved)
    last = enc.forward_cl(x)
    want = _fresh_like(enc, "BN").forward_cl(x)
    assert torch.equal(last, want)
    assert not torch.equal(last, first)


def test_pose_head_forms_follow_in_place_updates():
    from scflow_amd import ops
    from scflow_amd.modules import MultiClassPoseHead
    from tests.posehead_cases import ENC_CASES
    n, h, w, c0, c1 = ENC_CASES[0][0][:5]  # the batch-1 case at the decoder's smallest map
    assert n == 1

    def build(seed):
        head = MultiClassPoseHead(21, c0 + c1, "Basic", dict(type="GN", num_groups=32),
                                  dict(type="ReLU"), feat_size=(h, w), rotation_mode="ortho6d")
        synthetic.fill_module_(head, seed)
        return head.cuda()

    g = torch.Generator().manual_seed(8)
    s0 = torch.relu(torch.randn(n * h * w, c0, generator=g)).cuda()
    s1 = torch.relu(torch.randn(n * h * w, c1, generator=g)).cuda()
    label = torch.tensor([7], device="cuda")

    def run(head):
        r, t = head.forward_hip(ops.Chan.whole(s0), ops.Chan.whole(s1), n, h, w, label)
        return r.clone(), t.clone()

    head, fresh = build(7), build(3)
    fresh.load_state_dict(head.state_dict())
    first = run(head)
    for a, b in zip(first, run(fresh)):
        assert torch.equal(a, b)
    with torch.no_grad():
        for p in head.parameters():
            p.mul_(1.01)
    fresh = build(3)
    fresh.load_state_dict(head.state_dict())
    second = run(head)
    for a, b in zip(second, run(fresh)):
        assert torch.equal(a, b)
    assert not torch.equal(second[0], first[0])
    # each layer holds one packing, in the format of the kernel it runs on, plus FC1's permutation
    assert set(vars(head)["_derived"]) == {("enc_conv", 0), ("enc_conv", 1), ("ph_conv", 2),
                                           ("fc1", 128, 16)}


def test_a_recorded_launch_outlives_another_launch_shape():
    """``args`` at w = 32, ``run`` at w = 64, then the w = 32 struct again: it still points at the
    runner's live w = 32 form."""
    from scflow_amd import _lib, ops
    from scflow_amd.modules import ConvRunner
    conv = torch.nn.Conv2d(32, 32, 3, padding=1)
    synthetic.fill_module_(conv, 4)
    r = ConvRunner([conv.cuda()], "ReLU")
    g = torch.Generator().manual_seed(2)
    n, h = 1, 8
    x32, x64 = (torch.randn(n * h * w, 32, generator=g).cuda() for w in (32, 64))
    y32, y64 = torch.zeros(n * h * 32, 32, device="cuda"), torch.zeros(n * h * 64, 32, device="cuda")
    a32 = r.args(ops.Chan.whole(x32), ops.Chan.whole(y32), n, h, 32)
    launch = ops.BoundCall(_lib.load().scflow_conv2d, (ctypes.byref(a32),), 0, "scflow_conv2d")
    form32 = r.packed(32, 0, 32, a32.bk)[0]
    assert a32.weight == form32.data_ptr()
    launch()
    first = y32.clone()
    assert first.abs().max() > 0
    r.run(ops.Chan.whole(x64), ops.Chan.whole(y64), n, h, 64)
    assert r.packed(32, 0, 32, a32.bk)[0] is form32 and a32.weight == form32.data_ptr()
    y32.zero_()
    launch()
    torch.cuda.synchronize()
    assert torch.equal(y32, first)


def test_a_conv_struct_holds_what_it_points_at():
    """``conv2d_args`` attaches the packed weights and the bias to the struct: with every other
    reference dropped, and buffers of their sizes allocated and overwritten in between, the
    struct still launches the conv it was built for."""
    import gc
    from scflow_amd import ops
    conv = torch.nn.Conv2d(32, 32, 3, padding=1)
    synthetic.fill_module_(conv, 4)
    weight, bias0 = conv.weight.detach().cuda(), conv.bias.detach().cuda()
    n, h, w = 1, 8, 32
    x = torch.randn(n * h * w, 32, generator=torch.Generator().manual_seed(2)).cuda()
    bk = ops.conv_pick_bk(n, h, w, 32, 0, 32, 3, 3, 1, 1)

    def build(y):
        packed, bias = ops.pack_conv_weight(weight, 32, 0, w, 1, bk), bias0.clone()
        return ops.conv2d_args(ops.Chan.whole(x), packed, bias, n, h, w, 32, 3, 3, 1, 1, "ReLU",
                               out=ops.Chan.whole(y), bk=bk), packed.numel(), bias.numel()

    y, y_fresh = torch.zeros(n * h * w, 32, device="cuda"), torch.zeros(n * h * w, 32, device="cuda")
    a, n_packed, n_bias = build(y)
    torch.cuda.synchronize()
    gc.collect()
    # what the allocator would hand out again had the struct not held its inputs
    junk = [torch.full((size,), 1e30, device="cuda") for size in (n_packed, n_bias) * 3]
    torch.cuda.synchronize()
    ops.conv2d_launch(a, x)
    ops.conv2d_launch(build(y_fresh)[0], x)
    torch.cuda.synchronize()
    assert y.abs().max() > 0 and torch.isfinite(y).all()
    assert torch.equal(y, y_fresh)
    del junk


@pytest.mark.parametrize("hoist", [False, True])
def test_a_recorded_gru_step_replays_the_eager_one(hoist):
    """``ConvGRU.step`` recorded once under ``ops.binding`` and replayed twice against three eager
    steps from the same state (1 × 32 × 32, the narrowest map these kernels take; with and without
    the hoisted context): the same hidden state bit for bit after each, and the ``gru_zr`` /
    ``gru_q`` hooks called start / stop around each launch on every pass."""
    from scflow_amd import ops
    from scflow_amd.modules import ConvGRU
    n, h, w, hc, cxt = 1, 32, 32, 128, 128
    M = n * h * w
    gru = ConvGRU(hc, 2 * hc, "SeqConv")  # x = context | motion
    synthetic.fill_module_(gru, 3)
    gru = gru.cuda()
    hx0 = torch.randn(M, 3 * hc, generator=torch.Generator().manual_seed(6)).cuda()
    hx0[:, :hc].tanh_()
    want = [("gru_zr", True), ("gru_zr", False), ("gru_q", True), ("gru_q", False)] * 2  # two stages

    def state():
        hx = hx0.clone()
        log = []
        hooks = {name: (lambda start, name=name: log.append((name, start))) for name in ("gru_zr", "gru_q")}
        cm = gru.context_map(ops.Chan(hx, hc, cxt), n, h, w) if hoist else None
        args = (ops.Chan.whole(hx), ops.Chan.whole(torch.zeros(M, hc, device="cuda")),
                ops.Chan.whole(torch.zeros(M, hc, device="cuda")), n, h, w)
        return hx, log, lambda: gru.step(*args, hooks=hooks, ctx_map=cm, cxt_channels=cxt)

    hx_e, log_e, eager = state()
    hx_r, log_r, step = state()
    calls = []
    for i in range(3):
        eager()
        if i == 0:
            with ops.binding(calls):  # records and runs
                step()
        else:
            for c in calls:
                c()
        torch.cuda.synchronize()
        assert torch.equal(hx_r, hx_e), i
        assert log_e == want * (i + 1) and log_r == log_e, i
    assert not torch.equal(hx_e[:, :hc], hx0[:, :hc]) and torch.equal(hx_e[:, hc:], hx0[:, hc:])
    # in the record each launch stands between its start and its stop
    assert [isinstance(c, ops.BoundCall) for c in calls] == [False, True, False] * 4
