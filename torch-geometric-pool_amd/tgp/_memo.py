"""Facts remembered per tensor OBJECT: "rows are sorted", CSR offsets, batch sizes, ...  Full-batch training hands the
same ``edge_index`` / ``batch`` in every step, so what a first call found out (a host round trip, a launch) is kept.

A remembered fact is valid while the weak reference still resolves to the very same tensor and its version counter has
not moved -- an in-place torch operation bumps it, and a dead tensor's recycled ``id`` or memory never matches.  What
this cannot notice is stated at :func:`clear_memos`.  Imports nothing from the package (every module may use it).
"""
from weakref import ref

_ALL = []  # every TensorMemo of the package


def stamp(t):
    """What identifies "this very tensor, as it is now"; tested by :func:`unchanged`."""
    return ref(t), t._version


def unchanged(stamp, t) -> bool:
    return stamp[0]() is t and stamp[1] == t._version


class TensorMemo:
    """At most ``cap`` values, each stored for a key tensor, optionally together with a second tensor (the weights of an
    edge list) and a hashable ``extra`` (a node count).  A value stored without a second tensor is found only when asked
    for without one.  Values are whatever the caller stores except None, which is what a miss returns."""

    __slots__ = ("cap", "_d")

    def __init__(self, cap: int):
        self.cap = cap
        self._d = {}  # id(t) -> (ref(t), version, ref(other) | None, its version, extra, value), oldest first
        _ALL.append(self)

    def get(self, t, other=None, extra=None):
        e = self._d.get(id(t))
        if (e is not None and e[0]() is t and e[1] == t._version and e[4] == extra
                and (other is None if e[2] is None else (e[2]() is other and e[3] == other._version))):
            return e[5]
        return None

    def put(self, t, value, other=None, extra=None) -> None:
        """Stored at the young end; when full, the oldest entry goes.  An entry goes at once when its key tensor dies
        (a weak-reference callback: a dead list must not keep a device tensor alive, and no store scans for it)."""
        d, key = self._d, id(t)

        def forget(r):
            e = d.get(key)
            if e is not None and e[0] is r:
                del d[key]

        d.pop(key, None)
        while len(d) >= self.cap:
            d.pop(next(iter(d), None), None)
        d[key] = (ref(t, forget), t._version) + ((None, None) if other is None else stamp(other)) + (extra, value)

    def other(self, t):
        """The second tensor the value of ``t`` was stored with (None: no value, stored without one, or it is gone)."""
        e = self._d.get(id(t))
        return e[2]() if e is not None and unchanged(e, t) and e[2] is not None else None

    def discard(self, t) -> None:
        self._d.pop(id(t), None)

    def pop(self, t, other=None, extra=None):
        value = self.get(t, other, extra)
        self._d.pop(id(t), None)
        return value

    def clear(self) -> None:
        self._d.clear()

    def __len__(self) -> int:
        return len(self._d)


def clear_memos() -> None:
    """Forget every per-tensor fact the package remembers (row order, coalescedness, symmetry, CSR offsets, per-graph
    edge ranges, batch sizes, ...).  The memos key on object identity and PyTorch's version counter, so they notice
    in-place torch operations and nothing else: a write through ``.data``, through a DLPack / NumPy alias or through a
    raw pointer into a reused buffer is not seen, and the facts of the old contents would be used for the new ones.
    Call this after such a write."""
    for memo in _ALL:
        memo.clear()
