"""The one cache of device stacks (_lib._StackCache) behind acquire_batch*, acquire_signals and acquire_along, driven
with stub objects - `_h`, `ctx`, `n`, a key and a counting close() - so no device is needed: per context, most recently
used last, at most two entries per context; a hit needs the same class, an equal key, a capacity of at least the
request and a live handle; eviction closes the oldest and nothing else."""
from wavelets_amd import _lib as L


class Stub:
    made = []

    def __init__(self, ctx, n, *key):
        self._h, self.ctx, self.n, self.key, self.closed = 1, ctx, n, key, 0
        Stub.made.append(self)

    def _key(self):
        return self.key

    def close(self):
        self._h = None
        self.closed += 1


class Other(Stub):
    pass


KEY = (64, L.B3SPLINE, 3)


def test_a_hit_pops_the_entry_and_a_miss_makes_a_new_one():
    c, ctx = L._StackCache(), object()
    a = Stub(ctx, 4, *KEY)
    c.release(a)
    assert c.lists[id(ctx)] == [a]
    assert c.acquire(Stub, ctx, 4, *KEY) is a and c.lists[id(ctx)] == []
    b = c.acquire(Stub, ctx, 4, *KEY)                                    # (taken out: not handed out twice)
    assert b is not a and type(b) is Stub and (b.ctx, b.n, b.key) == (ctx, 4, KEY) and b is Stub.made[-1]
    assert a.closed == b.closed == 0


def test_a_larger_stack_serves_a_smaller_request_and_not_the_other_way_round():
    c, ctx = L._StackCache(), object()
    a = Stub(ctx, 4, *KEY)
    c.release(a)
    assert c.acquire(Stub, ctx, 5, *KEY) is not a and c.lists[id(ctx)] == [a]
    assert c.acquire(Stub, ctx, 2, *KEY) is a


def test_another_key_or_class_misses():
    c, ctx = L._StackCache(), object()
    a = Stub(ctx, 4, *KEY)
    c.release(a)
    for key in ((65,) + KEY[1:], KEY[:1] + (L.TRIANGLE,) + KEY[2:], KEY[:2] + (4,), KEY + (True,)):
        assert c.acquire(Stub, ctx, 4, *key) is not a
    got = c.acquire(Other, ctx, 4, *KEY)
    assert got is not a and type(got) is Other
    c.release(got)
    assert type(c.acquire(Stub, ctx, 4, *KEY)) is Stub and c.lists[id(ctx)] == [got]          # a subclass is another class
    assert c.acquire(Other, ctx, 4, *KEY) is got and a.closed == 0


def test_a_third_release_closes_the_oldest_and_nothing_else():
    c, ctx = L._StackCache(), object()
    a, b, d = (Stub(ctx, 4, n, L.B3SPLINE, 3) for n in (16, 32, 64))
    c.release(a)
    c.release(b)
    assert (a.closed, b.closed) == (0, 0)
    c.release(d)
    assert (a.closed, b.closed, d.closed) == (1, 0, 0) and c.lists[id(ctx)] == [b, d] and c.MAX == 2
    # most recently used last: b is taken and given back, so d is now the oldest
    assert c.acquire(Stub, ctx, 1, 32, L.B3SPLINE, 3) is b
    c.release(b)
    e = Stub(ctx, 4, 128, L.B3SPLINE, 3)
    c.release(e)
    assert (a.closed, b.closed, d.closed, e.closed) == (1, 0, 1, 0) and c.lists[id(ctx)] == [b, e]


def test_a_closed_entry_is_never_handed_out_nor_taken_in():
    c, ctx = L._StackCache(), object()
    a = Stub(ctx, 4, *KEY)
    c.release(a)
    a.close()
    assert c.acquire(Stub, ctx, 4, *KEY) is not a
    c.release(None)
    dead = Stub(ctx, 4, *KEY)
    dead.close()
    c.release(dead)
    assert dead not in c.lists[id(ctx)] and dead.closed == 1


def test_two_contexts_do_not_see_each_others_entries():
    c, one, two = L._StackCache(), object(), object()
    a, b = Stub(one, 4, *KEY), Stub(two, 4, *KEY)
    c.release(a)
    assert c.acquire(Stub, two, 4, *KEY) is not a
    c.release(b)
    for ctx in (one, two):                       # the limit is per context
        c.release(Stub(ctx, 4, *KEY))
    assert (a.closed, b.closed) == (0, 0)
    assert c.acquire(Stub, two, 4, *KEY).ctx is two and c.acquire(Stub, one, 4, *KEY).ctx is one


def test_the_three_module_caches_are_distinct_and_the_public_names_go_through_them(monkeypatch):
    caches = (L._batch_cache, L._signal_cache, L._along_cache)
    assert all(type(c) is L._StackCache for c in caches) and len({id(c) for c in caches}) == 3
    assert len({id(c.lists) for c in caches}) == 3
    fresh = {name: L._StackCache() for name in ("_batch_cache", "_signal_cache", "_along_cache")}
    for name, c in fresh.items():
        monkeypatch.setattr(L, name, c)
    ctx = object()
    stubs = [Stub(ctx, 4, *KEY) for _ in range(3)]
    for s, release in zip(stubs, (L.release_batch, L.release_signals, L.release_along)):
        for _ in range(3):                       # three releases into one cache evict nothing from the other two
            release(Stub(ctx, 1, 8, L.B3SPLINE, 1))
        release(s)
    assert [c.lists[id(ctx)][-1] for c in fresh.values()] == stubs and not any(s.closed for s in stubs)
    assert L.release_batch64 is L.release_batch and L.release_rl_batch64 is L.release_batch
    for trim, s in zip((L.trim_batches, L.trim_signals, L.trim_along), stubs):
        trim()
        assert [t.closed for t in stubs] == [int(t is s or stubs.index(t) < stubs.index(s)) for t in stubs]


def test_trim_closes_everything_once():
    c, one, two = L._StackCache(), object(), object()
    held = [Stub(ctx, 4, n, L.B3SPLINE, 3) for ctx in (one, two) for n in (16, 32)]
    for s in held:
        c.release(s)
    c.trim()
    assert [s.closed for s in held] == [1] * 4 and c.lists == {}
    c.trim()
    assert [s.closed for s in held] == [1] * 4
