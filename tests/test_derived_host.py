"""CPU: the rule of ``scflow_amd/derived.py`` — when a weight-derived form is made again — on its
own, with CPU tensors and counting ``make``s; and the sites whose keys it replaced
(``ConvRunner.packed``, ``graph._param_versions``, the encoder's eval-BatchNorm affine)."""
import pytest
import torch
import torch.nn as nn

from scflow_amd import derived as dv
from scflow_amd.derived import bump_weights_generation, derived, stamp


class _Owner:
    pass


class _Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return object()


def test_hit_and_miss_rules():
    o, make = _Owner(), _Counter()
    p = nn.Parameter(torch.zeros(4))
    first = derived(o, "k", (p,), make)
    assert derived(o, "k", (p,), make) is first and make.n == 1  # same key, same stamp: a hit
    with torch.no_grad():
        p.add_(1)
    second = derived(o, "k", (p,), make)
    assert make.n == 2 and second is not first  # an in-place write moves the version counter
    p.data = torch.ones(4)
    derived(o, "k", (p,), make)
    assert make.n == 3  # new storage
    derived(o, "k", (p, None), make)
    assert make.n == 4  # None among the tensors is accepted (and is another stamp than without)
    assert derived(o, "k", (p, None), make) is derived(o, "k", (p, None), make) and make.n == 4
    derived(o, "k", (p, torch.zeros(1)), make)
    assert make.n == 5  # the None turned into a tensor
    # a write that autograd does not see (it stands in for a replayed graph): the counter did not
    # move, so this is a hit — by the rule such a writer announces itself ...
    kept = derived(o, "k", (p,), make)
    n = make.n
    p.data.copy_(torch.full((4,), 7.0))
    assert derived(o, "k", (p,), make) is kept and make.n == n
    # ... through the generation
    p.data.copy_(torch.full((4,), 8.0))
    bump_weights_generation()
    assert derived(o, "k", (p,), make) is not kept and make.n == n + 1
    p.grad = torch.ones(4)
    torch.optim.SGD([p], lr=0.1).step()
    derived(o, "k", (p,), make)
    assert make.n == n + 2  # an optimizer step


def test_stamp_format():
    p, q = torch.zeros(2), torch.zeros(3)
    assert stamp(p, None, q) == ((p.data_ptr(), p._version), None, (q.data_ptr(), q._version),
                                 dv.weights_generation())
    assert stamp() == (dv.weights_generation(),)


def test_keys_coexist_and_stale_entries_leave_together():
    o, make = _Owner(), _Counter()
    p = nn.Parameter(torch.zeros(4))
    a, b = derived(o, "a", (p,), make), derived(o, "b", (p,), make)
    assert a is not b and make.n == 2
    assert derived(o, "a", (p,), make) is a and derived(o, "b", (p,), make) is b and make.n == 2
    forms = vars(o)["_derived"]
    assert set(forms) == {"a", "b"} and [k for k in vars(o)] == ["_derived"]  # one attribute
    old = stamp(p)
    for _ in range(3):  # repeated steps do not grow the dict
        with torch.no_grad():
            p.add_(1)
        derived(o, "a", (p,), make)
        assert set(forms) == {"a"} and forms["a"][0] == stamp(p) != old
    assert derived(o, "b", (p,), make) is not b
    assert set(forms) == {"a", "b"} and all(s == stamp(p) for s, _ in forms.values())


def test_an_entry_of_an_intermediate_stamp_leaves_too():
    """a made at stamp 0, b at stamp 1, a again at stamp 2: b is stale and goes; an entry made from
    other tensors stays."""
    o, make = _Owner(), _Counter()
    p, q = nn.Parameter(torch.zeros(4)), nn.Parameter(torch.zeros(4))
    derived(o, "a", (p,), make)
    other = derived(o, "other", (q,), make)
    with torch.no_grad():
        p.add_(1)
    derived(o, "b", (p,), make)
    with torch.no_grad():
        p.add_(1)
    derived(o, "a", (p,), make)
    assert set(vars(o)["_derived"]) == {"a", "other"}
    assert derived(o, "other", (q,), make) is other


def test_a_failed_make_leaves_no_entry():
    o = _Owner()

    def make():
        raise ValueError("no form")
    with pytest.raises(ValueError):
        derived(o, "k", (torch.zeros(1),), make)
    assert vars(o)["_derived"] == {}


def test_lib_reexports_the_generation():
    from scflow_amd import _lib
    g = _lib.weights_generation()
    _lib.bump_weights_generation()
    assert dv.weights_generation() == _lib.weights_generation() == g + 1


# ---------------------------------------------------------------------------------- the sites
@pytest.fixture()
def packs(monkeypatch):
    """``ops.pack_conv_weight`` replaced by a counting fake (CPU): the calls' arguments."""
    from scflow_amd import ops
    calls = []

    def fake(wt, c0, c1, w, stride, bk):
        calls.append((c0, c1, w, stride, bk))
        return wt.clone()
    monkeypatch.setattr(ops, "pack_conv_weight", fake)
    return calls


def test_conv_runner_holds_one_form_per_launch_shape(packs):
    from scflow_amd.modules import ConvRunner
    conv = nn.Conv2d(32, 32, 3, padding=1)
    r = ConvRunner([conv], "ReLU")
    p32 = r.packed(32, 0, 32, 16)
    p64 = r.packed(32, 0, 64, 16)
    again = r.packed(32, 0, 32, 16)
    assert len(packs) == 2 and packs == [(32, 0, 32, 1, 16), (32, 0, 64, 1, 16)]
    assert again is p32 and again[0] is p32[0] and p64[0] is not p32[0]
    assert torch.equal(p32[1], conv.bias.detach())
    with torch.no_grad():
        conv.bias.add_(1)  # a bias update re-makes the bias
    q32 = r.packed(32, 0, 32, 16)
    assert q32[1] is not p32[1] and torch.equal(q32[1], conv.bias.detach())
    assert set(vars(r)["_derived"]) == {(32, 0, 32, 16)}  # the w = 64 form of the old bias left too
    assert r._bk is None and r._bk_shape is None and not r.winograd and not r.wino4


def test_conv_runner_refuses_convs_with_and_without_bias(packs):
    from scflow_amd.modules import ConvRunner
    r = ConvRunner([nn.Conv2d(32, 32, 3, padding=1), nn.Conv2d(32, 32, 3, padding=1, bias=False)], None)
    with pytest.raises(ValueError):
        r.packed(32, 0, 32, 16)
    # with the bias folded elsewhere the mix is allowed, as before
    r = ConvRunner(r.convs, None, with_bias=False)
    assert r.packed(32, 0, 32, 16)[1] is None


def test_param_versions_is_the_stamp_over_the_state_dict():
    from scflow_amd import graph
    m = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))
    want = stamp(*m.state_dict().values())
    assert graph._param_versions(m) == want and len(want) == len(m.state_dict()) + 1
    with torch.no_grad():
        m[0].weight.mul_(2)
    assert graph._param_versions(m) != want
    assert graph._param_versions(m) == stamp(*m.state_dict().values())


def test_marking_running_statistics_as_written_remakes_the_bn_affine():
    """What the training BatchNorm does after its launch (``increment_version`` on the running
    statistics it wrote through raw pointers) changes the stamp ``_bn_affine`` keys its form by."""
    from scflow_amd import encoder
    bn = nn.BatchNorm2d(8).eval()
    with torch.no_grad():
        bn.running_var.uniform_(0.5, 2.0)
        bn.running_mean.normal_()
    before = stamp(*encoder._bn_tensors(bn))
    a = encoder._bn_affine(bn)
    assert encoder._bn_affine(bn) is a
    assert vars(bn)["_derived"]["affine"][0] == before  # the stamp _bn_affine itself took
    bn.running_mean.data.mul_(2)  # a raw write: not seen ...
    assert encoder._bn_affine(bn) is a
    for t in (bn.running_mean, bn.running_var):
        torch.autograd.graph.increment_version(t)  # ... until it is marked
    assert stamp(*encoder._bn_tensors(bn)) != before
    b = encoder._bn_affine(bn)
    assert b is not a and vars(bn)["_derived"]["affine"][0] == stamp(*encoder._bn_tensors(bn))
    sc = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    torch.testing.assert_close(b[0], sc.detach())
    torch.testing.assert_close(b[1], (bn.bias - bn.running_mean * sc).detach())


def test_batch_norm_nhwc_marks_what_its_launch_wrote(monkeypatch):
    """``batch_norm_nhwc`` moves the version counters of the running statistics (the launch is
    replaced by a no-op here: the marking is host-only)."""
    from scflow_amd.train import functions as fn
    bn = nn.BatchNorm2d(8)
    x = torch.zeros(2, 4, 4, 8)
    monkeypatch.setattr(fn._BatchNormNHWC, "apply", staticmethod(lambda x, *a: x))
    v = (bn.running_mean._version, bn.running_var._version)
    fn.batch_norm_nhwc(x, bn)
    assert (bn.running_mean._version, bn.running_var._version) == (v[0] + 1, v[1] + 1)
