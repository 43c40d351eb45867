"""The one staleness rule of everything the modules derive from parameters (packed weights, folded BatchNorm, host copies,
pack tables, captured graphs).  A derived value is stale once a source may have changed: ``_version`` shows in-place updates;
the parameter epoch shows what it misses -- every optimizer step (torch's fused optimizers leave ``_version`` alone), every
train() <-> eval() switch of a fused module, and ``bump_param_epoch()``, which code that writes parameters where ``_version``
cannot see it (``.data`` in-place writes, raw pointers) calls itself; and a replaced tensor is a new source even where pointer
and version match.  ``cached`` applies the rule to one value, ``module_stamp`` cheaply to a whole module tree."""
import functools
import itertools
import weakref

from torch.nn.modules.module import (register_module_buffer_registration_hook, register_module_module_registration_hook,
                                     register_module_parameter_registration_hook)
from torch.optim.optimizer import register_optimizer_step_post_hook

_epoch = [0]


def param_epoch():
    return _epoch[0]


def bump_param_epoch():
    _epoch[0] += 1


register_optimizer_step_post_hook(lambda optimizer, args, kwargs: bump_param_epoch())

# Advanced by every registration of a parameter, buffer or submodule anywhere (``m.w = nn.Parameter(...)``, assign=True loads,
# submodule swaps): ``module_stamp`` then re-reads its cached tensor list.
_structure = [0]


def _restructured(module, name, value):
    _structure[0] += 1


for _register in (register_module_parameter_registration_hook, register_module_buffer_registration_hook,
                  register_module_module_registration_hook):
    _register(_restructured)


def _key(tensors):
    return tuple((id(t), t.data_ptr(), t.shape, t._version) for t in tensors if t is not None) + (_epoch[0],)


def _expire(stamp, _):
    s = stamp()
    if s is not None:
        s.key = None


class Stamp:
    """Per tensor (None skipped) the object, pointer, shape and ``_version``, and the epoch.  Objects are held weakly and the
    death of any voids the stamp, so an equal ``id`` is the same object; the pointer implies the device (unified addressing)."""
    __slots__ = ("key", "refs", "__weakref__")

    def __init__(self, tensors):
        self.key = _key(tensors)
        expire = functools.partial(_expire, weakref.ref(self))
        self.refs = [weakref.ref(t, expire) for t in tensors if t is not None]

    def holds(self, tensors):
        return self.key == _key(tensors)

    def placed(self, tensors):
        """The same objects at the same addresses and shapes, whatever their values did since."""
        return self.key is not None and [k[:3] for k in self.key[:-1]] == [k[:3] for k in _key(tensors)[:-1]]


def cached(owner, slot, tensors, make):
    """``make()``, re-made only when the stamp of ``tensors`` no longer holds.  The value and its stamp live in
    ``owner.__dict__[slot]``, out of sight of ``nn.Module.__setattr__`` and ``state_dict``."""
    hit = owner.__dict__.get(slot)
    if hit is None or hit[0].key != _key(tensors):
        hit = owner.__dict__[slot] = (Stamp(tensors), make())
    return hit[1]


_lists = itertools.count()


def module_stamp(module):
    """Changes whenever a cache below ``module`` may be stale.  Walking the tree costs 1.6 ms for PSMNet's backbone, so the list
    of parameter and buffer objects is kept and re-read only after a registration; comparing it costs 0.1-0.15 ms."""
    d = module.__dict__
    c = d.get("_dmb_tensors")
    if c is None or c[0] != _structure[0]:
        tensors = list(module.parameters()) + list(module.buffers())
        same = c is not None and len(c[2]) == len(tensors) and all(a is b for a, b in zip(c[2], tensors))
        c = d["_dmb_tensors"] = (_structure[0], c[1] if same else next(_lists), tensors)
    return (_epoch[0], c[1]) + tuple((t.data_ptr(), t._version) for t in c[2])
