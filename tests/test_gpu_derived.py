"""GPU: weight-derived forms (``scflow_amd/derived.py``) follow the weights at every site that
keeps one — the encoders' packings and eval-BatchNorm affine, the pose head's per-layer packings
and FC1 permutation, ``ConvRunner``'s form per launch shape.  fp32 throughout; a module whose
weights moved must compute exactly what a freshly built module with those weights computes."""
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
    launch = ops.BoundLaunch(_lib.load().scflow_conv2d, a32, 0, "scflow_conv2d")
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
