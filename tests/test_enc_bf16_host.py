"""CPU: the bf16 direct 3×3 conv's RAFT-encoder form (SCFLOW_CONV_BF16_3X3N) as far as it goes
without a device — the launch plan through the host-only scflow_conv_plan_kind (fake aligned
pointers, nothing launched), the packed size, the Python knobs and the emulated oracle.  On the
parent commit ``_lib.CONV_BF16_3X3N`` does not exist, format 9 is SCFLOW_EINVAL and neither
``RAFTEncoder.bf16`` nor the refiners' ``enc_bf16`` exist."""
import ctypes
import os
import re

import pytest
import torch

from scflow_amd import _lib, ops
from tests import enc_bf16_restatement as er

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
SRC0, SRC1, WEIGHT, OUT, GATE, RH, HID, BMAP, ISC, ISH, OSC, OSH, RES = (0x10000 * (i + 1) for i in range(13))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every residual-stage channel count at every width a 256² or 512² image (and the 128² image's
# covered stages) gives it — a superset of the combinations that occur
ENC_SHAPES = [(c, w) for c in (64, 96, 128) for w in (32, 64, 128, 256)]
FUSED = {"plain": {}, "IN on load": dict(in_scale=ISC, in_shift=ISH),
         "BN affine": dict(out_scale=OSC, out_shift=OSH, act=1),
         "residual": dict(res=RES, sres=None),
         "BN affine + residual": dict(out_scale=OSC, out_shift=OSH, res=RES, sres=None, act=1),
         "all": dict(in_scale=ISC, in_shift=ISH, out_scale=OSC, out_shift=OSH, res=RES, sres=None, act=1)}


def conv(n, h, w, c0, c1, cout, k=3, bk=None, **over):
    kh, kw = (k, k) if isinstance(k, int) else k
    a = _lib.ConvArgs()
    a.src0, a.c0, a.s0 = SRC0, c0, c0
    if c1:
        a.src1, a.c1, a.s1 = SRC1, c1, c1
    a.weight, a.out, a.so = WEIGHT, OUT, cout
    a.n, a.h, a.w, a.cout = n, h, w, cout
    a.kh, a.kw, a.ph, a.pw, a.stride = kh, kw, kh // 2, kw // 2, 1
    a.bk = _lib.CONV_BF16_3X3N if bk is None else bk
    for key, v in over.items():
        setattr(a, key, cout if key == "sres" and v is None else v)
    return a


def kind(a):
    k = ctypes.c_int(-7)
    return _lib.load().scflow_conv_plan_kind(ctypes.byref(a), None, ctypes.byref(k)), k.value


def ws(a):
    return _lib.load().scflow_conv_workspace_bytes(ctypes.byref(a))


def test_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "scflow_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)\b", hdr).group(1))
    assert define("SCFLOW_CONV_BF16_3X3N") == _lib.CONV_BF16_3X3N == 9
    assert define("SCFLOW_PLAN_C3_BF16N") == _lib.PLAN_C3_BF16N == 16
    assert define("SCFLOW_CONV_BF16_3X3") == _lib.CONV_BF16_3X3 == 7
    assert define("SCFLOW_PLAN_C3_BF16") == _lib.PLAN_C3_BF16 == 15
    assert define("SCFLOW_CONV_BF16") == _lib.CONV_BF16 == 6
    assert define("SCFLOW_PLAN_SEP_BF16") == _lib.PLAN_SEP_BF16 == 14
    assert define("SCFLOW_ABI_VERSION") == _lib.ABI_VERSION == 4
    assert _lib.load().scflow_abi_version() == 4


# ------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("fused", list(FUSED), ids=list(FUSED))
@pytest.mark.parametrize("c,w", ENC_SHAPES)
def test_encoder_shapes_plan_the_encoder_form(c, w, fused):
    planned = (OK, _lib.PLAN_C3_BF16N)
    for n, h in ((1, w), (8, w), (1, 4)):  # square maps and H = 4: one row block
        a = conv(n, h, w, c, 0, c, **FUSED[fused])
        assert kind(a) == planned
        assert ws(a) == 0


def test_any_cout_and_two_sources_plan():
    for cout in (1, 2, 31, 33, 127, 129):
        assert kind(conv(2, 8, 96, 64, 0, cout)) == (OK, _lib.PLAN_C3_BF16N)
    assert kind(conv(2, 8, 32, 64, 32, 64)) == (OK, _lib.PLAN_C3_BF16N)
    assert kind(conv(2, 8, 32, 64, 32, 64, **FUSED["BN affine + residual"])) == (OK, _lib.PLAN_C3_BF16N)


@pytest.mark.parametrize("what,args", [
    ("1×5", conv(2, 32, 32, 128, 0, 128, (1, 5))),
    ("5×5", conv(2, 32, 32, 128, 0, 64, 5)),
    ("stride 2", conv(2, 32, 32, 128, 0, 64, stride=2)),
    ("pad 0", conv(2, 32, 32, 128, 0, 64, ph=0, pw=0)),
    ("W 16", conv(2, 16, 16, 128, 0, 128)),
    ("W 48", conv(2, 48, 48, 128, 0, 64)),
    ("H = 6", conv(2, 6, 32, 128, 0, 64)),
    ("c0 = 130", conv(2, 32, 32, 130, 0, 64)),
    ("c0 = 48", conv(2, 32, 32, 48, 0, 64)),
    ("c1 = 16", conv(2, 32, 32, 128, 16, 64)),
    ("GRU z|r epilogue", conv(2, 32, 32, 128, 128, 256, epilogue=_lib.EPI_GRU_ZR, gate=GATE, sg=128,
                              rh=RH, srh=128, hid=HID, sh=128, out=None)),
    ("GRU q epilogue", conv(2, 32, 32, 128, 128, 128, epilogue=_lib.EPI_GRU_Q, gate=GATE, sg=128,
                            hid=HID, sh=128, out=None)),
    ("bias map", conv(2, 32, 32, 128, 0, 64, bias_map=BMAP, sbm=64)),
    ("IN on load with a second source", conv(2, 32, 32, 64, 64, 64, in_scale=ISC, in_shift=ISH)),
    ("pixel stride below the channels", conv(2, 32, 32, 128, 0, 64, s0=96)),
    ("sources past 2 GiB of offsets", conv(128, 256, 256, 64, 0, 64)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_outside_the_domain_is_unsupported(what, args):
    assert kind(args) == (EUNSUPPORTED, _lib.PLAN_NONE), what
    assert ws(args) == EUNSUPPORTED, what


def test_half_an_affine_is_invalid():
    for over in (dict(in_scale=ISC), dict(in_shift=ISH), dict(out_scale=OSC), dict(out_shift=OSH),
                 dict(in_scale=ISC, in_shift=ISH, out_shift=OSH), dict(res=RES, sres=32)):
        a = conv(2, 32, 32, 64, 0, 64, **over)
        assert kind(a) == (EINVAL, _lib.PLAN_NONE), over
        assert ws(a) == EINVAL, over
    assert kind(conv(2, 32, 32, 64, 0, 64, out=None)) == (EINVAL, _lib.PLAN_NONE)


def test_alignment():
    assert kind(conv(2, 32, 32, 128, 0, 64, s0=386)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 32, 64, s1=34)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 0, 64, src0=SRC0 + 4)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 0, 64, res=RES, sres=66)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 0, 64, in_scale=ISC + 4, in_shift=ISH)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 0, 64, s0=388, res=RES, sres=68)) == (OK, _lib.PLAN_C3_BF16N)


def test_the_motion_encoder_format_keeps_its_domain():
    """SCFLOW_CONV_BF16_3X3 still refuses every fused piece and every width but 32 and 64."""
    seven = _lib.CONV_BF16_3X3
    assert kind(conv(2, 32, 32, 128, 0, 64, bk=seven)) == (OK, _lib.PLAN_C3_BF16)
    assert kind(conv(2, 64, 64, 128, 0, 64, bk=seven)) == (OK, _lib.PLAN_C3_BF16)
    for over in (dict(in_scale=ISC, in_shift=ISH), dict(out_scale=OSC, out_shift=OSH),
                 dict(res=RES, sres=64)):
        assert kind(conv(2, 32, 32, 128, 0, 64, bk=seven, **over)) == (EUNSUPPORTED, _lib.PLAN_NONE)
    for w in (48, 96, 128, 256):
        assert kind(conv(2, 8, w, 128, 0, 64, bk=seven)) == (EUNSUPPORTED, _lib.PLAN_NONE)
        assert _lib.load().scflow_conv_packed_size_bk(64, 128, 0, 3, 3, 1, w, seven) == EUNSUPPORTED
    assert kind(conv(2, 32, 32, 128, 0, 64, bk=_lib.CONV_BF16)) == (EUNSUPPORTED, _lib.PLAN_NONE)


def test_packed_size_equals_the_motion_encoder_formats():
    size = _lib.load().scflow_conv_packed_size_bk
    nine, seven = _lib.CONV_BF16_3X3N, _lib.CONV_BF16_3X3
    for c0, c1, cout in [(64, 0, 64), (96, 0, 96), (128, 0, 128), (32, 0, 33), (64, 32, 1)]:
        want = (cout + 31) // 32 * 32 * (c0 + c1) * 9 // 2
        for w in (32, 64):
            assert size(cout, c0, c1, 3, 3, 1, w, nine) == size(cout, c0, c1, 3, 3, 1, w, seven) == want
        for w in (96, 128, 256):
            assert size(cout, c0, c1, 3, 3, 1, w, nine) == want
    assert size(64, 128, 0, 5, 5, 1, 32, nine) == EUNSUPPORTED
    assert size(64, 128, 0, 3, 3, 2, 32, nine) == EUNSUPPORTED
    assert size(64, 130, 0, 3, 3, 1, 32, nine) == EUNSUPPORTED
    assert size(64, 128, 16, 3, 3, 1, 32, nine) == EUNSUPPORTED
    assert size(64, 128, 0, 3, 3, 1, 48, nine) == EUNSUPPORTED
    assert size(64, 128, 0, 3, 3, 1, 16, nine) == EUNSUPPORTED
    assert size(64, 128, 0, 3, 3, 1, 32, 5) == EINVAL  # 5 stays no format


def test_pick_bk_never_returns_the_format():
    for c, w in ENC_SHAPES:
        for n in (1, 2, 32, 64):
            bk = ops.conv_pick_bk(n, w, w, c, 0, c, 3, 3, 1, 1)
            assert bk in (8, 16, _lib.CONV_WINO, _lib.CONV_WINO4), (c, w, n, bk)


# ------------------------------------------------------------------------------------- the knobs
def _encoder(norm="IN"):
    from scflow_amd import MODELS
    return MODELS.build(dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic",
                             norm_cfg=dict(type=norm)))


def test_encoder_knob_defaults_to_fp32():
    from scflow_amd import encoder
    for norm in ("IN", "BN"):
        enc = _encoder(norm)
        assert enc.bf16 is False and enc.last_bf16 == ()
        assert "bf16" not in enc.state_dict() and not any("bf16" in k for k in enc.state_dict())
    assert encoder.BF16_STAGES == er.WIRED
    assert set(er.WIRED) <= {"res_layer1", "res_layer2", "res_layer3"}


def test_wired_conv_names():
    """``last_bf16``'s expected contents: the stride-1 3×3 convs of the wired stages, in launch
    order — never a first conv of a downsampling block."""
    names = er.wired_convs()
    assert len(names) == sum({"res_layer1": 4, "res_layer2": 3, "res_layer3": 3}[s] for s in er.WIRED)
    assert "res_layer2.0.conv1" not in names and "res_layer3.0.conv1" not in names
    enc = _encoder()
    for nm in names:
        c = enc.get_submodule(nm)
        assert c.kernel_size == (3, 3) and c.stride == (1, 1)


def test_refiner_knob_sets_every_encoder_and_clears():
    from scflow_amd import MODELS
    from scflow_amd.refiner import _RefinerBase
    from tests.test_gpu_decoder import decoder_cfg
    enc = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic", norm_cfg=dict(type="IN"))
    ctx = dict(type="RAFTEncoder", in_channels=3, out_channels=256, net_type="Basic", norm_cfg=dict(type="BN"))
    for sep in (False, True):
        r = MODELS.build(dict(type="SCFlowRefiner", cxt_channels=128, h_channels=128, seperate_encoder=sep,
                              encoder=enc, cxt_encoder=ctx,
                              decoder=dict(type="SCFlowDecoder", **decoder_cfg(2))))
        assert isinstance(r, _RefinerBase) and r.enc_bf16 is False
        encs = (r.real_encoder, r.render_encoder, r.context)
        assert all(e.bf16 is False for e in encs)
        r.enc_bf16 = True
        r._set_enc_bf16()
        assert all(e.bf16 is True for e in encs)
        assert r.decoder.gru_bf16 is False and r.decoder.menc_bf16 is False  # independent knobs
        r.enc_bf16 = False
        r._set_enc_bf16()
        assert all(e.bf16 is False for e in encs)
        assert not any("bf16" in k for k in r.state_dict())


def test_every_refiner_has_the_knob():
    import inspect

    from scflow_amd import raft_refiner, refiner
    for cls in (refiner.SCFlowRefiner, raft_refiner.RAFTRefinerFlow, raft_refiner.RAFTRefinerFlowMask):
        assert issubclass(cls, refiner._RefinerBase)
        assert cls.extract_feat is refiner._RefinerBase.extract_feat
        assert cls._features_into_hx is refiner._RefinerBase._features_into_hx
    src = inspect.getsource(refiner._RefinerBase)
    assert src.count("self._set_enc_bf16()") == 2  # extract_feat and the fused path


def test_training_never_selects_the_format():
    src = open(os.path.join(ROOT, "scflow_amd", "train", "model.py")).read()
    assert "BF16" not in src and "enc_bf16" not in src and ".bf16" not in src


# ------------------------------------------------------------------------------------- the oracle
def test_restated_launch_is_the_plain_conv_on_exact_data():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (2, 4, 6, 5), generator=g).float()
    w = torch.randint(-1, 2, (3, 4, 3, 3), generator=g).float()
    b = torch.randint(-4, 5, (3,), generator=g).float() / 4
    sc = torch.tensor([[0.5, 1, 2, 1], [2, 2, 0.5, 1]])
    sh = torch.randint(-3, 4, (2, 4), generator=g).float()
    osc, osh = torch.tensor([0.5, 1.0, 2.0]), torch.tensor([0.25, -1.0, 3.0])
    res = torch.randint(-8, 9, (2, 3, 6, 5), generator=g).float()
    xin = torch.relu(x * sc[:, :, None, None] + sh[:, :, None, None])
    want = torch.relu(torch.nn.functional.conv2d(xin, w, b, padding=1) * osc[None, :, None, None] +
                      osh[None, :, None, None] + res)
    got = er.launch(x, w, b, sc, sh, osc, osh, res, "ReLU")
    assert got.dtype == torch.float64 and torch.equal(got.float(), want)
    # zero padding pads the normalised activation: a positive shift must not leak into the border
    ones = torch.ones(1, 1, 3, 3)
    y = er.launch(torch.zeros(1, 1, 4, 4), ones, None, torch.ones(1, 1), torch.full((1, 1), 2.0))
    assert y[0, 0, 0, 0] == 8 and y[0, 0, 1, 1] == 18


def test_emulation_differs_from_the_fp32_oracle_and_is_removed_again():
    from oracle import scflow_oracle as orc
    from tests.helpers import encoder_state_dict
    plain = orc._basic_block
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 3, 64, 64, generator=g)
    for norm, seed in (("IN", 1), ("BN", 2)):
        sd = encoder_state_dict(norm, seed)
        ref = orc.raft_encoder(sd, x, norm)
        with er.emulating():
            assert orc._basic_block is er.basic_block_bf16
            emu = orc.raft_encoder(sd, x, norm)
        assert orc._basic_block is plain
        assert torch.isfinite(emu).all() and emu.shape == ref.shape
        if er.WIRED:
            assert not torch.equal(emu, ref), norm
        assert torch.equal(orc.raft_encoder(sd, x, norm), ref)
    with pytest.raises(RuntimeError):
        with er.emulating():
            raise RuntimeError("inside")
    assert orc._basic_block is plain


def test_emulation_rounds_only_the_wired_stride_1_convs():
    """Scaling a weight by 1 + 2⁻¹³ (a 16th of a bf16 half-ulp) after it has been made
    bf16-representable is rounded away where the emulation rounds and seen where it does not."""
    from tests.helpers import encoder_state_dict
    from oracle import scflow_oracle as orc
    sd = {k: (er.round_bf16(v) if k.endswith("weight") and v.dim() == 4 else v)
          for k, v in encoder_state_dict("BN", 2).items()}
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(5))
    tiny = 1 + 2 ** -13

    def run(key=None):
        d = dict(sd)
        if key is not None:
            d[key] = sd[key] * tiny
        with er.emulating():
            return orc.raft_encoder(d, x, "BN")
    base = run()
    rounded = [nm + ".weight" for nm in er.wired_convs()]
    exact = ["conv1.weight", "conv2.weight", "res_layer2.0.conv1.weight", "res_layer3.0.conv1.weight",
             "res_layer2.0.downsample.0.weight", "res_layer3.0.downsample.0.weight"]
    exact += [f"{s}.{b}.conv{i}.weight" for s in ("res_layer1", "res_layer2", "res_layer3")
              if s not in er.WIRED for b in (0, 1) for i in (1, 2)]
    for key in rounded:
        assert torch.equal(run(key), base), key
    for key in set(exact) - set(rounded):
        assert not torch.equal(run(key), base), key
