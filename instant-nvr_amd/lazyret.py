"""LazyDict: a dict that still owes some of its entries.

The return dicts of Renderer.render promise entries they have not made yet: the frame behind them may still be in flight
(renderer.LazyHostRet / LazyDevRet), raw / occ may still be on the device (LazyHostRet), the training tensors may still be in the
workspace (autograd.LazyTrainRet).  The reference's callers treat all of them as plain dicts, so ONE rule holds for every way of
looking at such a dict, and it is stated here once: what is promised is resolved before it is looked at —
  * by key (`[]`, get, pop, setdefault, del): that key only; `in` and len() answer from the promise without resolving anything,
  * as a whole (keys / items / values, iteration, reversed, copy, ==, !=, popitem, |, pickling, and with them dict(ret)): everything.
copy(), | and pickling / copy.deepcopy yield a plain dict.

A subclass states two things: `_promised()`, the keys it still owes (none of them stored yet), and `_resolve(keys=None)`, which
stores the owed entries among `keys` (None: all of them) with dict.__setitem__ / dict.update.
"""


class LazyDict(dict):
    def _promised(self):
        return ()

    def _resolve(self, keys=None):
        pass

    def _plain(self):
        self._resolve()
        return dict(dict.items(self))

    # ---- by key ----
    def __contains__(self, k):
        return dict.__contains__(self, k) or k in self._promised()

    def __len__(self):
        return dict.__len__(self) + len(self._promised())

    def __getitem__(self, k):
        self._resolve((k,))
        return dict.__getitem__(self, k)

    def __delitem__(self, k):
        self._resolve((k,))
        dict.__delitem__(self, k)

    def get(self, k, d=None):
        return self[k] if k in self else d

    def pop(self, k, *default):
        self._resolve((k,))
        return dict.pop(self, k, *default)

    def setdefault(self, k, d=None):
        self._resolve((k,))
        return dict.setdefault(self, k, d)

    # ---- as a whole (dict's C fast paths — dict(ret), {**ret} — go through keys() and [] once __iter__ is overridden) ----
    def keys(self):
        self._resolve()
        return dict.keys(self)

    def items(self):
        self._resolve()
        return dict.items(self)

    def values(self):
        self._resolve()
        return dict.values(self)

    def __iter__(self):
        self._resolve()
        return dict.__iter__(self)

    def __reversed__(self):
        self._resolve()
        return dict.__reversed__(self)

    def popitem(self):
        self._resolve()
        return dict.popitem(self)

    def copy(self):
        return self._plain()

    def __eq__(self, other):
        self._resolve()
        return dict.__eq__(self, other._plain() if isinstance(other, LazyDict) else other)

    def __ne__(self, other):
        eq = self.__eq__(other)
        return eq if eq is NotImplemented else not eq

    __hash__ = None

    def __or__(self, other):
        return self._plain() | (other._plain() if isinstance(other, LazyDict) else other)

    def __ror__(self, other):
        return other | self._plain()

    def __ior__(self, other):
        self._resolve()
        return dict.__ior__(self, other)

    def __reduce__(self):                       # pickle / copy.deepcopy
        return (dict, (self._plain(),))

    def __repr__(self):
        return '%s(%s%s)' % (type(self).__name__, dict.__repr__(self), ''.join(', %s: <on first access>' % k for k in self._promised()))
