"""feed.ResidentBagCache without a GPU: the arena lives on the CPU device and ops.bag_gather is replaced by a recorded
torch restatement (torch.cat of the sources, converted by torch, into the leading rows of each destination).

Checked: under one torch.manual_seed the cache visits the dataset indices the bare loader visits, in its order, for
sequential, shuffled and weighted samplers, over three epochs, and leaves the torch RNG where the bare loader leaves it;
hits + misses == len(loader) every epoch; admission is first come, never evicted, and says so in stats(); arena slots
are 256-byte aligned and disjoint; sentinels and event_time come out as DevicePrefetcher hands them on; a bf16 store
delivers x.to(bfloat16).float() in every epoch; RankShard of a cache yields the rank's positions and keeps the rank's
cache; and the grouped holders take resident bags by reference -- one gather per buffer, per-bag copies only for the rest."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset, RandomSampler, SequentialSampler, WeightedRandomSampler

from multimodalfusion_amd import feed, ops
from multimodalfusion_amd.utils import core_utils

L = 16
ROWS = [5, 1, 9, 3, 7, 2, 8, 4, 6, 11, 10, 12]


class Subjects(Dataset):
    """In-memory subjects in the reference's tuple; subject 3 has no pathology bag (the zeros((1, 1)) sentinel)."""

    def __init__(self, rows=ROWS):
        g = torch.Generator().manual_seed(11)
        self.bags = [torch.randn(n, L, generator=g) for n in rows]
        self.seen = []

    def __len__(self):
        return len(self.bags)

    def __getitem__(self, i):
        self.seen.append(int(i))
        path = torch.zeros(1, 1) if i == 3 else self.bags[i]
        return ({"T1": self.bags[i] + 1.0, "T2": torch.zeros(1, 1)}, path, torch.full((1, 4), float(i), dtype=torch.float64),
                torch.tensor([i % 4]), np.array([float(10 + i)]), torch.tensor([float(i % 3 == 0)]))


def one(batch):
    return batch[0]


@pytest.fixture
def gathers(monkeypatch):
    calls = []

    def bag_gather(planes, dst):
        planes, dst = [list(p) for p in planes], list(dst)
        rows = sum(int(x.shape[0]) for x in planes[0])
        for p, d in zip(planes, dst):
            d[:rows].copy_(torch.cat(p).to(d.dtype))
        calls.append((len(planes), len(planes[0]), planes[0][0].dtype, dst[0].dtype))
        return [int(x.shape[0]) for x in planes[0]]

    monkeypatch.setattr(ops, "bag_gather", bag_gather)
    return calls


def cache_of(loader, **kw):
    kw.setdefault("capacity_bytes", 1 << 20)
    return feed.ResidentBagCache(loader, device="cpu", **kw)


def samplers(ds):
    w = torch.tensor([1.0, 5.0, 1.0, 1.0, 5.0, 1.0, 1.0, 1.0, 5.0, 1.0, 1.0, 1.0])
    return {"sequential": SequentialSampler(ds), "random": RandomSampler(ds),
            "weighted": WeightedRandomSampler(w, len(ds), replacement=True)}


@pytest.mark.parametrize("kind", ["sequential", "random", "weighted"])
def test_three_epochs_visit_what_the_bare_loader_visits(kind, gathers):
    def epochs(wrap):
        ds = Subjects()
        loader = DataLoader(ds, batch_size=1, sampler=samplers(ds)[kind], collate_fn=one)
        src = wrap(loader)
        torch.manual_seed(1234)
        visited, per_epoch = [], []
        for _ in range(3):
            before = dict(src.stats()) if hasattr(src, "stats") else None
            visited.append([int(b[2][0, 0]) for b in src])
            if before is not None:
                after = src.stats()
                per_epoch.append((after["hits"] - before["hits"], after["misses"] - before["misses"]))
        return visited, per_epoch, torch.get_rng_state(), ds, src

    bare, _, rng_bare, _, _ = epochs(lambda ld: ld)
    got, per_epoch, rng_cache, ds, cache = epochs(cache_of)
    assert got == bare
    assert torch.equal(rng_cache, rng_bare)                       # the torch RNG was consumed exactly as by the loader
    assert all(h + m == len(ROWS) for h, m in per_epoch), per_epoch
    # every subject was read from the dataset once, when first drawn (a duplicate in its first epoch hits already)
    first = list(dict.fromkeys(i for ep in bare for i in ep))
    assert ds.seen == first
    assert cache.stats()["misses"] == len(first) and cache.stats()["refused"] == 0
    if kind == "weighted":
        assert len(set(bare[0])) < len(bare[0])                   # the case has duplicates at all
    if kind == "sequential":
        assert per_epoch == [(0, 12), (12, 0), (12, 0)]


def test_values_sentinels_and_event_time_come_out_as_from_the_prefetcher(gathers):
    ds = Subjects()
    cache = cache_of(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=one))
    for epoch in range(2):
        for i, (radio, path, genomic, label, event_time, c) in enumerate(cache):
            want = Subjects()[i]
            assert list(radio) == ["T1", "T2"] and torch.equal(radio["T1"], want[0]["T1"])
            assert tuple(radio["T2"].shape) == (1, 1) and not radio["T2"].any()
            assert torch.equal(path, want[1]) and path.dtype == torch.float32
            assert (tuple(path.shape) == (1, 1)) == (i == 3)
            assert genomic.dtype == torch.float32 and torch.equal(genomic, want[2].float())       # .float(), as there
            assert torch.equal(label, want[3]) and label.dtype == torch.int64 and torch.equal(c, want[5])
            assert isinstance(event_time, np.ndarray) and event_time == want[4]                   # handed on untouched
    assert gathers == []                                          # kept as delivered: views of the arena, no launch


def _slots(cache):
    out = []
    for it in cache.items.values():
        out += [(t.data_ptr(), t.numel() * t.element_size()) for t in it.leaves if torch.is_tensor(t)]
    return sorted(out)


def test_arena_slots_are_aligned_and_disjoint(gathers):
    cache = cache_of(DataLoader(Subjects(), batch_size=1, shuffle=True, collate_fn=one))
    list(cache)
    slots = _slots(cache)
    assert len(slots) == 12 * 6
    assert all(p % 256 == 0 for p, _ in slots)
    assert all(p + n <= q for (p, n), (q, _) in zip(slots, slots[1:]))
    lo, hi = cache.arena.slabs[0].data_ptr(), cache.arena.slabs[0].data_ptr() + cache.arena.slabs[0].numel()
    assert len(cache.arena.slabs) == 1 and all(lo <= p and p + n <= hi for p, n in slots)
    assert cache.stats()["resident_bytes"] == sum((n + 255) // 256 * 256 for _, n in slots) <= cache.capacity_bytes


def test_first_come_admission_never_evicts(gathers):
    rows = [8] * 6
    need = 2 * 8 * L * 4 + 4 * 256          # one subject: two [8 x L] fp32 bags, and a 256-byte slot for each small tensor
    ds = Subjects(rows)
    cache = cache_of(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=one), capacity_bytes=3 * need + need // 2)
    for epoch in range(3):
        got = [int(b[2][0, 0]) for b in cache]
        assert got == list(range(6))
        assert sorted(cache.items) == [(0,), (1,), (2,)]                     # the first three that fit, for good
        s = cache.stats()
        assert (s["hits"], s["misses"]) == (3 * epoch, 6 + 3 * epoch)
        assert s["items"] == 3 and s["refused"] == 3 and s["resident_bytes"] == 3 * need
    assert ds.seen == [0, 1, 2, 3, 4, 5] + [3, 4, 5] * 2                     # the others are loaded every epoch
    ptrs = _slots(cache)
    list(cache)
    assert _slots(cache) == ptrs


def test_a_refused_duplicate_is_loaded_once_per_epoch(gathers):
    ds = Subjects([8] * 4)
    sampler = [0, 1, 1, 0, 1]               # a fixed order with repeats (any iterable of indices is a sampler)
    cache = cache_of(DataLoader(ds, batch_size=1, sampler=sampler, collate_fn=one),
                     capacity_bytes=2 * 8 * L * 4 + 4 * 256)
    assert [int(b[2][0, 0]) for b in cache] == sampler
    assert ds.seen == [0, 1] and cache.stats() == dict(hits=3, misses=2, items=1, refused=1,
                                                       resident_bytes=2 * 8 * L * 4 + 4 * 256)
    assert [int(b[2][0, 0]) for b in cache] == sampler
    assert ds.seen == [0, 1, 1]


@pytest.mark.parametrize("path_dtype", [None, torch.bfloat16])
def test_bf16_store_delivers_the_same_values_every_epoch(path_dtype, gathers):
    ds = Subjects()
    cache = cache_of(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=one), store_dtype=torch.bfloat16)
    cache.path_dtype = path_dtype           # what a wrapped DevicePrefetcher(path_dtype=...) hands over
    for epoch in range(2):
        for i, (radio, path, genomic, *_rest) in enumerate(cache):
            assert torch.equal(radio["T1"], (ds.bags[i] + 1.0).to(torch.bfloat16).float())
            if i == 3:
                assert tuple(path.shape) == (1, 1) and path.dtype == torch.float32
            elif path_dtype is None:
                assert torch.equal(path, ds.bags[i].to(torch.bfloat16).float())
                assert path._mmf_resident.dtype == torch.bfloat16           # widened from its arena view
            else:
                assert path.dtype == torch.bfloat16 and path._mmf_resident is True      # a bf16 consumer gets the view
                assert torch.equal(path, ds.bags[i].to(torch.bfloat16))
            assert genomic.dtype == torch.float32                                   # small tensors are kept as they are
    n_bags, n_path = 12, 11
    narrowed = n_bags + n_path
    widened = 2 * (n_bags + (n_path if path_dtype is None else 0))
    assert len(gathers) == narrowed + widened
    assert gathers.count((1, 1, torch.float32, torch.bfloat16)) == narrowed
    up = lambda n: (n + 255) // 256 * 256
    # half the bytes per bag: T1 and (but for the sentinel of subject 3) the pathology bag in bf16, four small slots
    assert cache.stats()["resident_bytes"] == sum(up(n * L * 2) * (1 if i == 3 else 2) + (5 if i == 3 else 4) * 256
                                                  for i, n in enumerate(ROWS))


@pytest.mark.parametrize("wrapped", ["loader", "sequence", "iterable"])
def test_rank_shard_of_a_cache(wrapped, gathers):
    ds = Subjects()
    if wrapped == "loader":
        src = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=one)
    elif wrapped == "sequence":
        src = [ds[i] for i in range(len(ds))]
    else:
        class Sized:
            def __len__(self):
                return len(ds)

            def __iter__(self):
                return (ds[i] for i in range(len(ds)))
        src = Sized()
    cache = cache_of(src)
    for rank in range(3):
        for epoch in range(2):
            shard = feed.RankShard(cache, rank, 3)
            got = [int(b[2][0, 0]) for b in shard]
            assert shard.n_total == 12 and got == list(range(rank, 12, 3)) == [shard.position(i) for i in range(4)]
        sub = cache.shard(rank, 3, None)                        # the rank's cache outlives the epoch's RankShard
        assert sub.stats()["hits"] == 4 and sub.stats()["misses"] == 4
    assert cache.stats()["items"] == 0


def test_position_keys_for_a_sequence(gathers):
    ds = Subjects()
    seq = [ds[i] for i in range(len(ds))]
    cache = cache_of(seq)
    for epoch in range(2):
        assert [int(b[2][0, 0]) for b in cache] == list(range(12))
    assert sorted(cache.items) == list(range(12)) and cache.stats()["hits"] == 12


# ---- the grouped holders take resident bags by reference ----------------------------------------------------------
def _copies(monkeypatch):
    n = {"copy_": 0}
    real = torch.Tensor.copy_

    def copy_(self, *a, **k):
        n["copy_"] += 1
        return real(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "copy_", copy_)
    return n


def test_held_bags_gather_a_resident_window_in_one_call(gathers, monkeypatch):
    ds = Subjects()
    cache = cache_of(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=one))
    batches = [b for b in cache if tuple(b[1].shape) != (1, 1)][:5]
    held = core_utils._HeldBags()
    n = _copies(monkeypatch)
    lab = torch.tensor([0])
    never = lambda: pytest.fail("nothing to flush")
    for slot, b in enumerate(batches):
        held.add([b[1]], lab, lab.float(), slot, 10 ** 6, torch.device("cpu"), never)
    assert n["copy_"] == 0 and gathers == []                   # held by reference until the grouped call runs

    class PathHead:
        pass
    x, sizes = held.held(PathHead())
    assert gathers == [(1, 5, torch.float32, torch.float32)]   # one launch for the window
    monkeypatch.undo()
    assert sizes == [int(b[1].shape[0]) for b in batches]
    assert torch.equal(x, torch.cat([b[1] for b in batches]))


def test_held_bags_mix_resident_and_other_bags(gathers, monkeypatch):
    ds = Subjects()
    cache = cache_of(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=one), store_dtype=torch.bfloat16)
    res = [b for b in cache][:3]
    host = [ds.bags[9], ds.bags[10]]
    gathers.clear()
    held = core_utils._HeldBags()
    lab = torch.tensor([0])
    order = [res[0][0]["T1"], host[0], res[1][0]["T1"], res[2][0]["T1"], host[1]]
    n = _copies(monkeypatch)
    for slot, x in enumerate(order):
        held.add([x, x], lab, lab.float(), slot, 10 ** 6, torch.device("cpu"), lambda: None)
    copies_in_add = n["copy_"]

    class RadioHead:
        attention_net_radio = None
    x, sizes = held.held(RadioHead())
    monkeypatch.undo()
    # the two host bags: one copy_ per plane each (plus the buffer's growth); the resident ones: one gather per run, both
    # planes in it, widened from the bf16 arena on the way
    assert gathers == [(2, 1, torch.bfloat16, torch.float32), (2, 2, torch.bfloat16, torch.float32)]
    assert 4 <= copies_in_add <= 4 + 4
    want = torch.cat(order)
    assert x.shape == (2, want.shape[0], L) and torch.equal(x[0], want) and torch.equal(x[1], want)
