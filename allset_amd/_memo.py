"""Data derived from a tensor, kept ON that tensor: the one caching idiom of the package.  A value lives in its
owner's ``__dict__`` and is served only to the very Python object it was stored for, while that object's version counter, address, shape
and dtype are what they were then (a :class:`Stamp`): it cannot be mistaken for another tensor at a recycled address and dies with its
owner -- so a value must not hold its owner strongly.  What no stamp can see is a write through ``t.data`` into the same storage
(``weight.data.uniform_()``, a raw-pointer optimizer kernel): data derived from tensors that are written that way belongs to the step
that built it (``dense.prefetch_wide_planes``), not here."""
import weakref

MISS = object()          # lookup(): nothing valid stored (None is a value)


class Stamp:
    __slots__ = ("ref", "state")

    def __init__(self, t):
        self.ref, self.state = weakref.ref(t), (t._version, t.data_ptr(), t.shape, t.dtype)

    def holds(self, t) -> bool:
        return self.ref() is t and self.state == (t._version, t.data_ptr(), t.shape, t.dtype)


class _Table(dict):       # (slot, key) -> (Stamp, value); copy.deepcopy and pickling take a tensor's __dict__ along: the copy starts empty
    def __reduce__(self):
        return _Table, ()


def lookup(t, slot: str, key=(), default=MISS):
    """The value stored on ``t`` under (slot, key) if it is still valid, else ``default``.  Reads only: it builds nothing and touches no
    device, so it is safe during graph capture."""
    entry = t.__dict__.get("_allset_memo", {}).get((slot, key))
    return entry[1] if (entry is not None and entry[0].holds(t)) else default


def get(t, slot: str, key, build):
    """:func:`lookup`, or ``build()`` stored for next time.  The stamp is taken AFTER the builder ran (it may update ``t`` in place);
    entries that an update of ``t`` has invalidated are dropped on the way."""
    value = lookup(t, slot, key)
    if value is MISS:
        value = build()
        table = t.__dict__["_allset_memo"] = _Table((k, e) for k, e in t.__dict__.get("_allset_memo", {}).items() if e[0].holds(t))
        table[(slot, key)] = (Stamp(t), value)
    return value
