"""GPU: feed.ResidentBagCache under the training loop.  Two epochs through the cache and two epochs through
feed.DevicePrefetcher, from the same seeds over a shuffled DataLoader, must leave every parameter equal BIT FOR BIT after
each epoch and log equal losses and risks: the cache changes where a bag comes from, not one value of it.  Grouped and
per-bag loops, a cache that holds about half the subjects, the radiology head (four planes in one gather), the multimodal
concat head, and a bf16-stored cache against a loader of bags rounded by torch.  In the second epoch of a grouped run
every window is ONE ops.bag_gather and no resident bag is copied on its own."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

from oracle import inputs as gen

pytestmark = pytest.mark.gpu

MODS = ["T1", "T2", "T1Gd", "FLAIR"]
PATH = [300, 1, 41, 128, 9, 250, 64, 77, 200, 17, 33, 5]
RADIO = [40, 8, 96, 1, 30, 64, 17, 50, 12, 72, 3, 25]
K = 4


class Subjects(Dataset):
    def __init__(self, head, rounded=False):
        rnd = (lambda t: t.to(torch.bfloat16).float()) if rounded else (lambda t: t)
        self.items = []
        for i, (n, r) in enumerate(zip(PATH, RADIO)):
            if head == "path":
                radio = {"T1": torch.zeros(1, 1)}
            else:
                radio = {m: rnd(torch.as_tensor(gen.bag(700 + i, r, stream=7 * j))) for j, m in enumerate(MODS)}
            path = torch.zeros(1, 1) if head == "radio" else rnd(torch.as_tensor(gen.bag(900 + i, n, stream=100)))
            omic = torch.as_tensor(gen.normal(500 + i, (1, 80), stream=200)) if head == "mm" else torch.zeros(1, 4)
            self.items.append((radio, path, omic, torch.tensor([i % K]), np.array([float(10 + i)]),
                               torch.tensor([float(i % 3 == 0)])))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _one(batch):
    return batch[0]


def _model(head):
    from multimodalfusion_amd import models
    if head == "path":
        sd = gen.path_state_dict(seed=515, gated=True, size="small", n_classes=K, dropout=True, bias_std=0.05)
        model = models.MIL_Attention_fc_surv_path(gate_path=True, model_size_wsi="small", dropout=True, n_classes=K)
    elif head == "radio":
        sd = gen.radio_state_dict(seed=616, gated=True, n_classes=K, dropout=True, n_mod=4, bias_std=0.05)
        model = models.MIL_Attention_fc_surv_radio(radio_fusion="concat", gate_radio=True, dropout=True, n_classes=K,
                                                   modalities=MODS)
    else:
        sd = gen.mm_state_dict(seed=616, input_dim=80, fusion="concat", gate_path=True, gate_radio=True, dropout=True,
                               n_classes=K, mode="radio_path_omic", n_mod=4, bias_std=0.05)
        model = models.MM_MIL_Attention_fc_surv(input_dim=80, radio_fusion="concat", fusion="concat", gate=True,
                                                gate_path=True, gate_omic=True, gate_radio=True, dropout=True,
                                                n_classes=K, mode="radio_path_omic")
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    model.relocate()
    return model


MODE = {"path": "path", "radio": "radio", "mm": "radio_path_omic"}


def _train(head, group, wrap, monkeypatch, rounded=False, each_epoch=None):
    """Two epochs of train_loop_survival over a shuffled DataLoader behind `wrap` -> per epoch (losses, risks, parameters)."""
    from multimodalfusion_amd import ops
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    model = _model(head)
    seeds = iter(range(9001, 9400))
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: next(seeds))
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    torch.manual_seed(2024)
    src = wrap(DataLoader(Subjects(head, rounded), batch_size=1, shuffle=True, collate_fn=_one))
    out = []
    for epoch in range(2):
        if each_epoch is not None:
            each_epoch(epoch, src)
        r = core_utils.train_loop_survival(epoch, model, src, opt, K, MODE[head], loss_fn=NLLSurvLoss(alpha=0.2), gc=4,
                                           group=group)
        torch.cuda.synchronize()
        out.append((r["losses"].copy(), r["risks"].copy(), {k: v.detach().clone() for k, v in model.state_dict().items()}))
    monkeypatch.undo()
    return out, src


def _same(got, want):
    for epoch, ((la, ra, pa), (lb, rb, pb)) in enumerate(zip(got, want)):
        assert np.array_equal(la, lb) and np.array_equal(ra, rb), epoch
        for k in pb:
            assert torch.equal(pa[k], pb[k]), (epoch, k)


def _bytes(head):
    """What the pathology head's subjects take in the arena: the bag, and a slot each for T1's sentinel, omic, label, c."""
    up = lambda n: (n + 255) // 256 * 256
    return sum(up(n * 4096) + 4 * 256 for n in PATH)


@pytest.mark.parametrize("head,group,capacity", [
    ("path", True, 64 << 20), ("path", False, 64 << 20), ("path", True, "half"), ("radio", True, 64 << 20),
    ("mm", True, 64 << 20)])
def test_training_through_the_cache_equals_training_through_the_prefetcher(head, group, capacity, monkeypatch):
    from multimodalfusion_amd import feed
    if capacity == "half":
        capacity = _bytes(head) // 2
    want, _ = _train(head, group, feed.DevicePrefetcher, monkeypatch)
    got, cache = _train(head, group, lambda ld: feed.ResidentBagCache(ld, capacity_bytes=capacity), monkeypatch)
    _same(got, want)
    s = cache.stats()
    assert s["hits"] + s["misses"] == 24
    if capacity == 64 << 20:
        assert (s["hits"], s["misses"], s["items"], s["refused"]) == (12, 12, 12, 0)
    else:
        assert 0 < s["items"] < 12 and s["refused"] == 12 - s["items"] and s["hits"] == s["items"]
        assert s["resident_bytes"] <= capacity


def test_a_bf16_stored_cache_trains_as_on_bags_rounded_by_torch(monkeypatch):
    """store_dtype=torch.bfloat16: the grouped windows are widened out of the arena by the gather itself, in the first
    epoch too, to exactly x.to(bfloat16).float()."""
    from multimodalfusion_amd import feed
    want, _ = _train("path", True, feed.DevicePrefetcher, monkeypatch, rounded=True)
    got, cache = _train("path", True, lambda ld: feed.ResidentBagCache(ld, capacity_bytes=64 << 20,
                                                                        store_dtype=torch.bfloat16), monkeypatch)
    _same(got, want)
    up = lambda n: (n + 255) // 256 * 256
    assert cache.stats()["resident_bytes"] == sum(up(n * 2048) + 4 * 256 for n in PATH)       # half the bytes per bag


@pytest.mark.parametrize("head", ["path", "radio"])
def test_the_second_epoch_is_one_gather_per_window(head, monkeypatch):
    from multimodalfusion_amd import feed, ops
    n = {"gather": [], "group": 0, "bag_copies": 0}
    gather0, copy0 = ops.bag_gather, torch.Tensor.copy_
    step = "amil_nll_step_group" if head == "path" else "radio_nll_step_group"
    step0 = getattr(ops, step)

    def each_epoch(epoch, src):
        if epoch != 1:
            return

        def gather(planes, dst):
            n["gather"].append((len(planes), len(planes[0])))
            return gather0(planes, dst)

        def group_step(*a, **k):
            n["group"] += 1
            return step0(*a, **k)

        def copy_(self, src, *a, **k):
            if torch.is_tensor(src) and src.dim() >= 2 and src.shape[-1] == 1024:
                n["bag_copies"] += 1
            return copy0(self, src, *a, **k)

        monkeypatch.setattr(ops, "bag_gather", gather)
        monkeypatch.setattr(ops, step, group_step)
        monkeypatch.setattr(torch.Tensor, "copy_", copy_)

    _, cache = _train(head, True, lambda ld: feed.ResidentBagCache(ld, capacity_bytes=64 << 20), monkeypatch,
                      each_epoch=each_epoch)
    assert cache.stats()["hits"] == 12
    assert n["group"] == 3 and n["gather"] == [(1 if head == "path" else 4, 4)] * 3      # gc = 4: one launch per window
    assert n["bag_copies"] == 0                                                         # no resident bag is copied alone


@pytest.mark.parametrize("head", ["path", "radio"])
def test_a_bf16_store_delivers_the_same_values_in_every_epoch(head):
    from multimodalfusion_amd import feed
    ds = Subjects(head)
    cache = feed.ResidentBagCache(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=_one), capacity_bytes=64 << 20,
                                  store_dtype=torch.bfloat16)
    for epoch in range(2):
        for (radio, path, omic, label, event_time, c), want in zip(cache, ds.items):
            bags = [(path, want[1])] if head == "path" else [(radio[m], want[0][m]) for m in MODS]
            for got, x in bags:
                assert got.is_cuda and got.dtype == torch.float32
                assert torch.equal(got.cpu().view(torch.int32), x.to(torch.bfloat16).float().view(torch.int32)), epoch
            assert torch.equal(label.cpu(), want[3]) and torch.equal(c.cpu(), want[5]) and event_time is want[4]
    assert cache.stats()["hits"] == 12 and cache.stats()["misses"] == 12
