"""The policy of a TerrainWorld's chunk cache (DESIGN §4l "Cache and memory", §4p "The eroded world"), restated as plainly as
it can be: lists and sets of (layer, key), no buffers, no device.  Slow on purpose.

    One LRU over both layers: 'e', the chunks a request reads, and 'r', the raw chunks an eroded chunk is made from (its
    nine neighbours, row-major; a plain world's chunks have no sources and its raw layer stays empty).
    A call names the keys of one step.  A key that is resident is used; a missing one is made from its sources, which are
    used or made first.  Before anything is made, the least recently used entries outside "this call's keys, the last
    call's keys (the pinned ones) and the current chunk's sources" leave until the new entry fits -- or none is left.
    After the call, entries outside this call's keys leave in the same order until the budget holds.
"""


def nine_around(key):
    a, b = key
    return [(a + i, b + j) for i in (-1, 0, 1) for j in (-1, 0, 1)]


class CacheModel:
    def __init__(self, capacity, eroded):
        self.capacity, self.eroded = capacity, eroded
        self.lru = []                                             # (layer, key), least recently used first
        self.pinned = set()                                       # the last call's keys
        self.made = []                                            # (layer, key) of everything made so far, in order

    def resident(self, layer):
        return {k for l, k in self.lru if l == layer}

    def _use(self, entry):
        if entry in self.lru:
            self.lru.remove(entry)
        self.lru.append(entry)

    def _shrink(self, size, protected):
        for entry in [e for e in self.lru if e not in protected]:
            if size <= self.capacity:
                return
            self.lru.remove(entry)
            size -= 1

    def _make(self, entry, protected):
        self._shrink(len(self.lru) + 1, protected)
        self.made.append(entry)
        self._use(entry)

    def acquire(self, keys):
        step = {('e', k) for k in keys} | {('e', k) for k in self.pinned}
        for k in keys:
            if ('e', k) in self.lru:
                self._use(('e', k))
                continue
            sources = [('r', s) for s in nine_around(k)] if self.eroded else []
            for s in sources:
                if s in self.lru:
                    self._use(s)
                else:
                    self._make(s, step | set(sources))
            self._make(('e', k), step | set(sources))
        self.pinned = set(keys)
        self._shrink(len(self.lru), {('e', k) for k in keys})
