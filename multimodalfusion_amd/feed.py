"""Bag feed: host -> HBM staging of the next bag overlapped with the current bag's kernels.

The reference copies every tensor of a batch synchronously at the top of each iteration
(utils/core_utils.py:194-198: `.to(device)` on pageable memory).  At ~1 ms of GPU work per 50k bag the 205 MB copy
(~3.3 ms over PCIe Gen5 x16) dominates, so the feed keeps `depth` bags in flight: pinned host staging buffers, copies
issued with non_blocking=True on a dedicated HIP stream, an event per bag that the compute stream waits on.

`DevicePrefetcher(loader)` wraps any iterable that yields the reference's batch tuple
(radio_features: dict, path_features, genomic_features, label, event_time, c) -- e.g. a DataLoader built with
collate_MIL_survival (utils/utils.py:35-46) -- and yields the same tuple with the tensors already on the GPU.
"""
from __future__ import annotations

from collections import deque

import torch


def load_slide_bags(paths, pin: bool = True, dtype=None) -> torch.Tensor:
    """One subject's pathology bag from its per-slide `.pt` files, as datasets/dataset_survival.py:359-366 builds it
    (`torch.load` each slide, `torch.cat(dim=0)`), but assembled directly in ONE pinned host buffer: the slides are
    read into their row ranges, so there is no pageable intermediate and the H2D copy can be asynchronous.
    An empty list gives the reference's "missing" sentinel `torch.zeros((1, 1))` (dataset_survival.py:356-357).
    `dtype` (e.g. torch.bfloat16) narrows while copying -- meant for bags already stored in that type on disk, where
    it is a no-op; narrowing 200 MB of fp32 on the host costs more than the PCIe time it saves."""
    if len(paths) == 0:
        return torch.zeros((1, 1))
    bags = [torch.load(p, map_location="cpu") for p in paths]
    for b in bags:
        if b.dim() != 2 or b.shape[1] != bags[0].shape[1]:
            raise ValueError("slide bags must be [n_i x L] with one feature width")
    dt = dtype or bags[0].dtype
    out = torch.empty((sum(b.shape[0] for b in bags), bags[0].shape[1]), dtype=dt,
                      pin_memory=bool(pin) and torch.cuda.is_available())
    r = 0
    for b in bags:
        out[r:r + b.shape[0]].copy_(b)
        r += b.shape[0]
    return out


def intersect_modalities(features_by_mod, slice_index_by_mod, modalities=None, pin: bool = True, dtype=None,
                         require_equal: bool = True):
    """One subject's radiology bags restricted to the slices every modality has, as datasets/dataset_survival.py:346-348
    does it: `intersect = set.intersection(*[set(v) ...])`, then per modality the rows whose slice index is in the
    intersection, IN THEIR STORED ORDER (`features[np.in1d(slice_index, intersect), :]`).  Pure index work: the rows
    are gathered bit for bit.

    features_by_mod[m]: [n_m x 1024] array or tensor, slice_index_by_mod[m]: [n_m] slice ids (any integer or float type).
    `modalities` fixes the order of the returned dict (default: the order of `features_by_mod`; the reference iterates
    `self.modalities`).  Returns {m: tensor [n x 1024]} in ONE pinned host buffer per modality (what DevicePrefetcher copies
    asynchronously).  The model concatenates the modalities along the feature axis (models/model_attention_mil_radio.py:
    80-82), which needs equal n; a slice id that repeats inside one modality breaks that in the reference too (torch.cat
    raises there), so `require_equal` (default) raises ValueError here, at the point where the cause is still known."""
    import numpy as np
    mods = list(modalities) if modalities is not None else list(features_by_mod.keys())
    if not mods:
        return {}
    idx = {m: np.asarray(slice_index_by_mod[m]).reshape(-1) for m in mods}
    common = None
    for m in mods:
        u = np.unique(idx[m])
        common = u if common is None else np.intersect1d(common, u, assume_unique=True)
    out = {}
    for m in mods:
        f = features_by_mod[m]
        f = f if torch.is_tensor(f) else torch.as_tensor(np.asarray(f))
        if f.dim() != 2 or f.shape[0] != idx[m].shape[0]:
            raise ValueError(f"modality {m}: features {tuple(f.shape)} do not match {idx[m].shape[0]} slice ids")
        rows = torch.as_tensor(np.nonzero(np.isin(idx[m], common))[0])
        dst = torch.empty((rows.numel(), f.shape[1]), dtype=dtype or f.dtype,
                          pin_memory=bool(pin) and torch.cuda.is_available())
        if rows.numel():
            torch.index_select(f, 0, rows, out=dst) if dst.dtype == f.dtype else dst.copy_(f.index_select(0, rows))
        out[m] = dst
    if require_equal and len({t.shape[0] for t in out.values()}) > 1:
        raise ValueError("modalities keep different numbers of slices (a slice id repeats inside one modality): "
                         + ", ".join(f"{m}: {t.shape[0]}" for m, t in out.items()))
    return out


def load_radio_bags(h5_paths_by_mod, modalities=None, pin: bool = True, dtype=None):
    """datasets/dataset_survival.py:339-348 for one subject: read `features` and `slice_index` of every modality's .h5
    file, keep the common slices.  Needs h5py (absent from the build image: the read is three lines and untested here; the
    index work, which is what must be exact, is `intersect_modalities`)."""
    try:
        import h5py
    except ImportError as e:      # fail loudly, as everything on this path does
        raise ImportError("load_radio_bags needs h5py; pass arrays to feed.intersect_modalities instead") from e
    feats, idx = {}, {}
    for m, path in h5_paths_by_mod.items():
        with h5py.File(path, "r") as f:
            feats[m] = f["features"][:]
            idx[m] = f["slice_index"][:]
    return intersect_modalities(feats, idx, modalities, pin, dtype)


def _pin(t: torch.Tensor) -> torch.Tensor:
    if not torch.is_tensor(t) or t.is_cuda:
        return t
    return t if t.is_pinned() else t.pin_memory()


class DevicePrefetcher:
    def __init__(self, loader, device=None, depth: int = 2, path_dtype=None):
        """path_dtype=torch.bfloat16 delivers the pathology bag in bf16, which selects the bf16-storage kernels
        (include/mmf_amil.h: mmf_amil_bf16_*).  A bag that is already bf16 on the host crosses PCIe at half the
        bytes; an fp32 bag is copied as it is and narrowed on the device, on the copy stream."""
        self.loader = loader
        self.path_dtype = path_dtype
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.depth = max(1, int(depth))
        self.stream = torch.cuda.Stream(self.device)

    def __len__(self):
        return len(self.loader)

    def _stage(self, batch):
        radio, path, genomic, label, event_time, c = batch
        with torch.cuda.stream(self.stream):
            move = lambda t: _pin(t).to(self.device, non_blocking=True) if torch.is_tensor(t) else t
            path_d = move(path)
            if self.path_dtype is not None and torch.is_tensor(path_d) and path_d.dim() == 2 and path_d.shape[1] > 1 \
                    and path_d.dtype != self.path_dtype:
                path_d = path_d.to(self.path_dtype)          # on the copy stream, after the H2D of the fp32 bag
            out = ({k: move(v) for k, v in radio.items()}, path_d,
                   move(genomic.float() if torch.is_tensor(genomic) else genomic), move(label), event_time, move(c))
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return out, ev

    def __iter__(self):
        it = iter(self.loader)
        q = deque()
        try:
            for _ in range(self.depth):
                q.append(self._stage(next(it)))
        except StopIteration:
            pass
        while q:
            out, ev = q.popleft()
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)                       # compute waits for THIS bag only; later copies keep flowing
            for t in list(out[0].values()) + [out[1], out[2], out[3], out[5]]:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(cur)             # allocator: do not reuse before the compute stream is done
            try:
                q.append(self._stage(next(it)))
            except StopIteration:
                pass
            yield out


# ---- rank sharding of the training loader (one-bag-per-GPU data parallelism) ------------------------------------
class _StridedBatches(torch.utils.data.Sampler):
    """Batch sampler of rank r: every world-th batch of the base batch sampler's order for this epoch.  The order is
    drawn ONCE, on rank 0, and broadcast, so the ranks agree on it by construction (a RandomSampler draws its
    permutation from the global torch RNG, which nothing guarantees to be in the same state on every rank)."""

    def __init__(self, base, rank, world):
        self.base, self.rank, self.world = base, rank, world
        self.n_total = len(base)

    def __iter__(self):
        import torch.distributed as dist
        order = [list(b) for b in self.base] if self.rank == 0 else None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            box = [order]
            dist.broadcast_object_list(box, src=0)
            order = box[0]
        elif order is None:
            order = [list(b) for b in self.base]
        self.n_total = len(order)
        return iter(order[self.rank::self.world])

    def __len__(self):
        return (self.n_total - self.rank + self.world - 1) // self.world


class RankShard:
    """The part of `loader` that rank `rank` of `world` processes: loader positions rank, rank + world, ... --
    only those bags are read from disk, collated and copied.  Iterating yields the reference's batch tuples in
    position order; `n_total` is the length of the whole (unsharded) loader, `position(i)` the loader position of the
    i-th yielded batch.  Works for a torch DataLoader (a new DataLoader over the same dataset whose batch sampler is
    the strided view of the original one), for a DevicePrefetcher or a ResidentBagCache around one, for indexable sequences, and for any
    other sized iterable (there the skipped items are still produced by the iterable, then dropped)."""

    def __init__(self, loader, rank: int, world: int):
        self.rank, self.world = int(rank), int(world)
        self.n_total = len(loader)
        self._src = self._shard(loader)

    def _shard(self, loader):
        r, w = self.rank, self.world
        if isinstance(loader, DevicePrefetcher):
            return DevicePrefetcher(self._shard(loader.loader), loader.device, loader.depth, loader.path_dtype)
        if isinstance(loader, ResidentBagCache):
            return loader.shard(r, w, self._shard)       # the rank's own cache, kept from one epoch's RankShard to the next's
        if isinstance(loader, torch.utils.data.DataLoader):
            kw = dict(collate_fn=loader.collate_fn, num_workers=loader.num_workers, pin_memory=loader.pin_memory,
                      timeout=loader.timeout, worker_init_fn=loader.worker_init_fn)
            if loader.num_workers > 0:
                kw.update(prefetch_factor=loader.prefetch_factor, persistent_workers=loader.persistent_workers)
            return torch.utils.data.DataLoader(loader.dataset, batch_sampler=_StridedBatches(loader.batch_sampler, r, w), **kw)
        if hasattr(loader, "__getitem__"):
            return (loader[i] for i in range(r, self.n_total, w))
        import itertools
        return itertools.islice(iter(loader), r, None, w)

    def position(self, i: int) -> int:
        return self.rank + i * self.world

    def __iter__(self):
        return iter(self._src)


# ---- bags resident in HBM across epochs ----------------------------------------------------------------------------
def _rng_state(gen):
    return torch.get_rng_state() if gen is None else gen.get_state()


def _set_rng_state(gen, state):
    torch.set_rng_state(state) if gen is None else gen.set_state(state)


class _StridedIter:
    """Positions rank, rank + world, ... of a sized iterable, itself sized and iterable again every epoch."""

    def __init__(self, base, rank, world):
        self.base, self.rank, self.world = base, rank, world

    def __len__(self):
        return (len(self.base) - self.rank + self.world - 1) // self.world

    def __iter__(self):
        import itertools
        return itertools.islice(iter(self.base), self.rank, None, self.world)


class _StridedSeq(_StridedIter):
    """The same of an indexable sequence: only the rank's positions are ever read."""

    def __getitem__(self, i):
        return self.base[self.rank + i * self.world]

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class _Arena:
    """Device memory of a ResidentBagCache: a few large uint8 slabs, each taken once and never returned to the allocator
    while the cache lives, handed out by bump allocation at 256-byte alignment."""
    ALIGN = 256

    def __init__(self, capacity_bytes, device, slab_bytes=1 << 30):
        self.capacity, self.device, self.slab_bytes = int(capacity_bytes), device, int(slab_bytes)
        self.slabs, self.reserved, self.top, self.used = [], 0, 0, 0

    @classmethod
    def round_up(cls, n):
        return (int(n) + cls.ALIGN - 1) // cls.ALIGN * cls.ALIGN

    def take(self, nbytes):
        """A [nbytes] uint8 view (nbytes a multiple of ALIGN) at a 256-byte aligned address, or None: no room left."""
        if not self.slabs or self.top + nbytes > self.slabs[-1].numel():
            size = min(max(nbytes, self.slab_bytes), self.capacity - self.reserved)
            if size < nbytes:
                return None
            slab = torch.empty(size + self.ALIGN, dtype=torch.uint8, device=self.device)
            self.slabs.append(slab[(-slab.data_ptr()) % self.ALIGN:][:size])
            self.reserved += size
            self.top = 0
        out = self.slabs[-1][self.top:self.top + nbytes]
        self.top += nbytes
        self.used += nbytes
        return out


class _Resident:
    """One batch kept in the arena: its leaves (the radio modalities in the loader's order, then path, genomic, label, c --
    arena views, or whatever the loader gave where that was no tensor), the dtype each is delivered in, event_time, and
    the event recorded behind its copies."""
    __slots__ = ("names", "leaves", "deliver", "event_time", "event", "nbytes")


class ResidentBagCache:
    """Feeds a training or evaluation loop from HBM from the second epoch on: wraps whatever DevicePrefetcher wraps (or a
    DevicePrefetcher, whose path_dtype and loader it takes over) and yields the six-tuple a DevicePrefetcher around the
    same loader yields -- same tensors, same devices; sentinels and event_time handled as there -- but every batch it has
    seen stays on the device, in an arena of a few large slabs (bump allocation, 256-byte aligned, never freed).  Wrap the
    loader ONCE, outside the epoch loop: the cache is the state.

    Keys and order.  For a torch DataLoader the key of a batch is its dataset indices, and each epoch's order is drawn
    from the loader's own batch_sampler, consuming the torch RNG exactly as iterating the loader would (the iterator's
    base seed first, then the sampler's draws): shuffled and weighted samplers visit the same subjects in the same order
    with or without the cache, and an index drawn twice in one epoch (WeightedRandomSampler samples with replacement) hits
    the second time.  Indexable sequences and other sized iterables are keyed by POSITION, which is only right when
    their order is the same every epoch.

    Hits and misses.  A hit is served from the arena.  The misses of an epoch are loaded in order, ahead of need, by a
    DataLoader over just those batches (the _StridedBatches technique of RankShard) with the pinned, side-stream,
    event-per-batch staging of DevicePrefetcher, `depth` batches in flight, and are interleaved with the hits in epoch
    order.  A missed batch is admitted whenever it still fits in `capacity_bytes` (default: half of the free device
    memory at construction).  Nothing is ever evicted: under a cyclic scan of the epochs least-recently-used is the
    worst policy (every batch is thrown out just before it is needed again), and "whoever got in stays" keeps
    capacity / cohort of the epochs' traffic off PCIe.  A batch that does not fit flows through every epoch as it would
    through a DevicePrefetcher.  stats() counts hits, misses, resident bytes and the batches refused for space.

    Storage type.  store_dtype=None keeps a bag as it is delivered: its H2D copy lands directly in its arena slot, and
    the delivered tensor is a view of the arena -- no second copy, no launch.  store_dtype=torch.bfloat16 narrows fp32
    bags ([n x L], L % 8 == 0) into the arena with ops.bag_gather on the copy stream, so the same HBM holds twice the
    cohort.  That is LOSSY (round to nearest even) and opt-in; every delivery then widens out of the arena, in the first
    epoch too, so all epochs see the same values x.to(bfloat16).float() -- except a consumer that takes bf16 bags
    (path_dtype=torch.bfloat16 on the wrapped feed), which gets the view.  The delivered dtype follows the wrapped feed's
    path_dtype rule: the pathology bag in path_dtype when that is set, everything else as the loader gave it.

    Streams, as DevicePrefetcher: the compute stream waits for the batch's event; arena views need no record_stream
    (the arena is never freed); a widened temporary is made on the consuming stream.  A delivered bag carries the
    attribute `_mmf_resident` (True: it is an arena view; a tensor: the arena view it was widened from), by which the
    grouped loops take it by reference (utils/core_utils.py: _HeldBags)."""

    def __init__(self, loader, device=None, capacity_bytes=None, store_dtype=None, depth=2):
        self.path_dtype = None
        if isinstance(loader, DevicePrefetcher):
            self.path_dtype, device = loader.path_dtype, loader.device if device is None else device
            loader = loader.loader
        if store_dtype not in (None, torch.bfloat16):
            raise ValueError("store_dtype is None (keep as delivered) or torch.bfloat16")
        self.loader, self.store_dtype, self.depth = loader, store_dtype, max(1, int(depth))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        if capacity_bytes is None:
            capacity_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        self.capacity_bytes = int(capacity_bytes)
        self.arena = _Arena(self.capacity_bytes, self.device)
        self.items = {}
        self.hits = self.misses = 0
        self._refused = set()
        self._shards = {}

    def __len__(self):
        return len(self.loader)

    def stats(self):
        return dict(hits=self.hits, misses=self.misses, items=len(self.items), resident_bytes=self.arena.used,
                    refused=len(self._refused))

    def shard(self, rank, world, shard):
        """The cache of rank `rank` of `world` (RankShard): over `shard(self.loader)`, made once and kept, so that the
        rank's bags stay resident from one epoch's RankShard to the next's."""
        key = (int(rank), int(world))
        if key not in self._shards:
            ld = self.loader
            part = shard(ld) if isinstance(ld, torch.utils.data.DataLoader) \
                else (_StridedSeq if hasattr(ld, "__getitem__") else _StridedIter)(ld, key[0], key[1])
            sub = ResidentBagCache(part, self.device, self.capacity_bytes, self.store_dtype, self.depth)
            sub.path_dtype = self.path_dtype
            self._shards[key] = sub
        return self._shards[key]

    # -- the epoch's order ---------------------------------------------------------------------------------------
    def _sampled(self):
        ld = self.loader
        return isinstance(ld, torch.utils.data.DataLoader) and not isinstance(ld.dataset, torch.utils.data.IterableDataset)

    def _draw(self):
        """(keys, what to fetch a miss by) of this epoch, in order."""
        ld = self.loader
        if not self._sampled():
            return list(range(len(ld))), list(range(len(ld)))
        self._rng0 = _rng_state(ld.generator)
        torch.empty((), dtype=torch.int64).random_(generator=ld.generator)     # the base seed iter(loader) draws first
        if ld.batch_sampler is not None:
            fetch = [list(b) for b in ld.batch_sampler]
            return [tuple(b) for b in fetch], fetch
        fetch = list(ld.sampler)
        return fetch, fetch

    def _miss_iter(self, fetch, flags):
        """The epoch's missed batches (fetch[i] where flags[i]), host side, in order."""
        ld = self.loader
        if not any(flags):
            return iter(())
        if self._sampled():
            kw = dict(collate_fn=ld.collate_fn, num_workers=ld.num_workers, pin_memory=ld.pin_memory, timeout=ld.timeout,
                      worker_init_fn=ld.worker_init_fn, generator=ld.generator)
            if ld.num_workers > 0:
                kw.update(prefetch_factor=ld.prefetch_factor)
            want = [f for f, m in zip(fetch, flags) if m]
            sub = torch.utils.data.DataLoader(ld.dataset, batch_sampler=want, **kw) if ld.batch_sampler is not None \
                else torch.utils.data.DataLoader(ld.dataset, sampler=want, batch_size=None, **kw)
            after = _rng_state(ld.generator)
            _set_rng_state(ld.generator, self._rng0)     # its iterator draws the base seed the wrapped loader's would have
            it = iter(sub)
            _set_rng_state(ld.generator, after)
            return it
        if hasattr(ld, "__getitem__"):
            return (ld[i] for i, m in zip(fetch, flags) if m)
        import itertools
        return itertools.compress(iter(ld), flags)

    # -- staging ---------------------------------------------------------------------------------------------------
    def _on_copy_stream(self):
        import contextlib
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _event(self):
        if self.stream is None:
            return None
        ev = torch.cuda.Event()
        ev.record(self.stream)
        return ev

    def _stored_dtype(self, t, is_path):
        bag = t.dim() == 2 and t.shape[1] > 1
        if bag and t.dtype == torch.float32 and t.shape[1] % 8 == 0 and t.shape[0] >= 1 and (
                self.store_dtype == torch.bfloat16 or is_path and self.path_dtype == torch.bfloat16):
            return torch.bfloat16
        return t.dtype

    def _stage(self, key, batch):
        """Copies of one missed batch issued on the copy stream: into the arena when it fits (-> its _Resident, now in
        self.items), else as DevicePrefetcher stages it (-> the device tuple and its event)."""
        from . import ops
        radio, path, genomic, label, event_time, c = batch
        if torch.is_tensor(genomic):
            genomic = genomic.float()
        names = list(radio.keys())
        leaves = [radio[k] for k in names] + [path, genomic, label, c]
        i_path = len(names)
        pin = _pin if self.device.type == "cuda" else (lambda t: t)
        stored = [self._stored_dtype(t, i == i_path) if torch.is_tensor(t) else None for i, t in enumerate(leaves)]
        sizes = [_Arena.round_up(max(t.numel(), 1) * sd.itemsize) if sd is not None else 0 for t, sd in zip(leaves, stored)]
        block = self.arena.take(sum(sizes))
        with self._on_copy_stream():
            if block is None:
                self._refused.add(key)
                move = lambda t: pin(t).to(self.device, non_blocking=True) if torch.is_tensor(t) else t
                dev = [move(t) for t in leaves]
                p = dev[i_path]
                if self.path_dtype is not None and torch.is_tensor(p) and p.dim() == 2 and p.shape[1] > 1 \
                        and p.dtype != self.path_dtype:
                    dev[i_path] = p.to(self.path_dtype)
                out = (dict(zip(names, dev[:i_path])), dev[i_path], dev[i_path + 1], dev[i_path + 2], event_time,
                       dev[i_path + 3])
                return out, self._event()
            self._refused.discard(key)
            it = _Resident()
            it.names, it.event_time, it.nbytes, it.leaves, it.deliver = names, event_time, sum(sizes), [], []
            at = 0
            for i, (t, sd, nb) in enumerate(zip(leaves, stored, sizes)):
                if sd is None:
                    it.leaves.append(t)
                    it.deliver.append(None)
                    continue
                slot = block[at:at + t.numel() * sd.itemsize].view(sd).view(t.shape)
                at += nb
                if sd == t.dtype:
                    slot.copy_(pin(t), non_blocking=True)           # the H2D copy lands in the arena: no second copy
                else:
                    ops.bag_gather([[pin(t).to(self.device, non_blocking=True)]], [slot])      # narrowed on the copy stream
                slot._mmf_resident = True
                it.leaves.append(slot)
                it.deliver.append(self.path_dtype if i == i_path and self.path_dtype is not None and t.dim() == 2
                                  and t.shape[1] > 1 else t.dtype)
            it.event = self._event()
        self.items[key] = it
        return it, it.event

    def _deliver(self, it):
        """The six-tuple of a resident batch on the current stream."""
        from . import ops
        if it.event is not None:
            torch.cuda.current_stream(self.device).wait_event(it.event)
        out = []
        for t, dd in zip(it.leaves, it.deliver):
            if dd is not None and t.dtype != dd and t.shape[1] % 8:
                t = t.to(dd)                           # a width the gather does not take: the wrapped feed's conversion
            elif dd is not None and t.dtype != dd:     # a bf16-stored bag for an fp32 consumer: widened, exactly
                wide = torch.empty(t.shape, dtype=dd, device=t.device)
                ops.bag_gather([[t]], [wide])
                wide._mmf_resident = t
                t = wide
            out.append(t)
        n = len(it.names)
        return dict(zip(it.names, out[:n])), out[n], out[n + 1], out[n + 2], it.event_time, out[n + 3]

    def __iter__(self):
        keys, fetch = self._draw()
        left, flags, seen = {}, [], set()
        for k in keys:
            left[k] = left.get(k, 0) + 1
            flags.append(k not in self.items and k not in seen)
            seen.add(k)
        miss_keys = iter([k for k, m in zip(keys, flags) if m])
        host = self._miss_iter(fetch, flags)
        q, spill = deque(), {}

        def stage_next():
            try:
                batch = next(host)
            except StopIteration:
                return
            q.append(self._stage(next(miss_keys), batch))

        for _ in range(self.depth):
            stage_next()
        for k, miss in zip(keys, flags):
            left[k] -= 1
            if miss:
                self.misses += 1
                got, ev = q.popleft()
                stage_next()
            else:
                self.hits += 1
                got, ev = spill[k] if k in spill else (self.items[k], None)
            if isinstance(got, _Resident):
                yield self._deliver(got)
                continue
            # not resident (no room): through, as DevicePrefetcher delivers it; kept for a repeat later in this epoch
            if ev is not None:
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                for t in list(got[0].values()) + [got[1], got[2], got[3], got[5]]:
                    if torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(cur)
            if left[k]:
                spill[k] = (got, ev)
            else:
                spill.pop(k, None)
            yield got
