"""Weight-derived forms on the inference path: the one rule for when they are made again.

An inference module derives device buffers from its parameters — packed conv weights, the
permuted FC weight, the eval-BatchNorm affine, the XHead predictor table.  Each is made by a
launch or two and is valid for as long as the tensors it was made from hold the same values.
``derived`` keeps such forms; ``stamp`` is how it knows that the tensors still hold them.

The contract
------------
* ``stamp(*tensors)`` is ``(data_ptr(), _version)`` per tensor (``None`` for a ``None`` entry)
  plus ``weights_generation()``.  Two equal stamps mean: the same storage, no write that autograd
  saw, no write that announced itself through the generation.
* ``derived(owner, key, tensors, make)`` returns ``make()``'s value, made once per
  ``(key, stamp(*tensors))`` and kept in one dict on ``owner`` (a module or a runner) under the
  single attribute ``_derived``.  ``key`` names the form (a format, a launch shape): several keys
  live side by side under one stamp, so a runner holds one packing per launch shape and a struct
  recorded for one shape stays valid while another shape runs.  An entry whose stamp no longer
  matches is replaced, and the owner's other stale entries are dropped with it — every entry made
  from the same storages (the old stamp's or the new one's) under another stamp than the current
  one — so repeated optimizer steps do not grow the dict.  Entries made from other tensors (the
  pose head keeps one per layer on one owner) cannot be judged from here and wait for their own
  call.
* A hit costs one tuple build and one dict lookup.  Nothing here calls into ``torch.cuda``, walks
  a state dict, or knows about stream capture: a captured forward contains no pack launch
  because the warm-up before the capture filled the forms and the capture hits them.
* ``copy.deepcopy`` of an owner copies the dict, but the copied tensors live elsewhere, so the
  copied stamps match nothing and the forms are made again on first use.

The rule for writers that go around autograd
--------------------------------------------
A kernel that writes a parameter or buffer through its raw pointer leaves ``_version`` where it
was.  Such a writer either moves the version counter of what it wrote
(``torch.autograd.graph.increment_version``, host-only) — the training BatchNorm does that for
the running statistics it updates — or bumps the generation (``bump_weights_generation``) — the
replayed optimizer graph of ``train/step.py`` does that, since a replay passes no Python at all
per parameter.  A form keyed any other way would be stale after either; that is why the key is
built here and nowhere else.

The training path's counterpart is ``train/functions.py::_cached``.  It stays separate on
purpose: it lives on the weight *tensor*, not on a module (the GRU's concatenated weights are
made per step and take their forms with them when they die), and inside a hipGraph capture of
forward + backward it must *not* hit an eager form — the weights move between replays — so it has
a capture scope of its own.  Inference forms are made outside the graph and only read inside it.
"""
from __future__ import annotations

from typing import Any, Callable, Hashable, Optional, Sequence

import torch

_ATTR = "_derived"

# An update that does not move the version counters — a replayed hipGraph of the optimizer step
# (TrainStep(graph=True)) writes the parameters without autograd seeing it — bumps this instead.
_WEIGHTS_GEN = 0


def weights_generation() -> int:
    return _WEIGHTS_GEN


def bump_weights_generation() -> None:
    global _WEIGHTS_GEN
    _WEIGHTS_GEN += 1


def stamp(*tensors: Optional[torch.Tensor]) -> tuple:
    return tuple(None if t is None else (t.data_ptr(), t._version) for t in tensors) + (_WEIGHTS_GEN,)


def _storages(s: tuple) -> tuple:
    return tuple(e and e[0] for e in s[:-1])


def derived(owner: Any, key: Hashable, tensors: Sequence[Optional[torch.Tensor]],
            make: Callable[[], Any]) -> Any:
    forms = vars(owner).get(_ATTR)
    if forms is None:
        forms = vars(owner)[_ATTR] = {}
    now = stamp(*tensors)
    hit = forms.get(key)
    if hit is not None:
        if hit[0] == now:
            return hit[1]
        # stale with it: whatever else was made from these tensors (the storages of the old or of
        # the new stamp) under another stamp than the current one
        same = {_storages(hit[0]), _storages(now)}
        for k in [k for k, (s, _) in forms.items() if s != now and _storages(s) in same]:
            del forms[k]
    value = make()
    forms[key] = (now, value)
    return value
