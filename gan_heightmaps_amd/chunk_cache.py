"""The chunk cache of a TerrainWorld: equal-sized device buffers in layers ('e': the chunks a request reads,
'r': the raw ones an eroded chunk is made from) under ONE budget and ONE least-recently-used order, with a pool that recycles
the buffers of evicted chunks.  It knows nothing of what a chunk holds or how it is made -- the world's ``_acquire`` drives
it -- and needs ``alloc`` and ``free`` only."""
from collections import OrderedDict


class ChunkCache:
    def __init__(self, alloc, free, chunk_bytes, cache_mb):
        self.alloc, self.free, self.chunk_bytes, self.cache_mb = alloc, free, chunk_bytes, cache_mb
        self.layers = {'e': {}, 'r': {}}                          # layer -> {key: device pointer}
        self.order = OrderedDict()                                # the (layer, key) of every chunk, least recently used first
        self.pool, self.pinned = [], set()                        # buffers to use again; the last step's keys, kept in the next

    def capacity(self):
        return int(self.cache_mb * (1 << 20)) // self.chunk_bytes

    def buffer(self):
        """a chunk buffer for the caller to fill: a recycled one while there is one"""
        return self.pool.pop() if self.pool else self.alloc(self.chunk_bytes)

    def get(self, layer, key, keep, make):
        """use the chunk if it is resident; if not, make room for it outside ``keep`` first, then ``make()`` it"""
        if key in self.layers[layer]:
            self.order.move_to_end((layer, key))
        else:
            self.evict(keep, 1)
            self.layers[layer][key] = make()
            self.order[(layer, key)] = None

    def evict(self, keep, more=0):
        """the least recently used chunks outside ``keep`` (a set of (layer, key)) go to the pool until what is resident, and
        ``more`` chunks, fit the budget"""
        size, cap = len(self.order) + more, self.capacity()
        for layer, key in [lk for lk in self.order if lk not in keep]:
            if size <= cap:
                break
            self.pool.append(self.layers[layer].pop(key))
            del self.order[(layer, key)]
            size -= 1

    def drop(self):
        """every chunk goes to the pool; nothing is pinned"""
        for chunks in self.layers.values():
            self.pool.extend(chunks.values())
            chunks.clear()
        self.order.clear()
        self.pinned = set()

    def free_pool(self):                                          # (the caller has waited for what may still read them)
        for p in self.pool:
            self.free(p)
        self.pool = []
