"""feed.ResidentBagCache and ops.bag_gather, measured in one process.  One JSON line per case.

Gather leg, per window shape (device events, warm-up first, median of three):
  (a) gather_ms   ONE ops.bag_gather of the window out of bags scattered through an arena;
  (b) copies_ms   the G (x planes) copy_ calls into the same buffer -- what the holders do with device bags otherwise;
  (c) contig_ms   one contiguous copy_ of the same bytes: this box's copy rate;
  widen_ms        (a) out of a bf16 arena into the fp32 window; tb_s: bytes read + written by (a) per second.
  The bound: (a) < (b) for every window of G >= 16.  The yardstick, reported: (a) <= 1.10 x (c) + 0.015 ms.
End-to-end leg (wall clock around a synchronised epoch, median of three), bags/s of a loader over pinned host bags:
  one 50k x 1024 fp32 bag per step (model.nll_step), and 64 x 1k grouped windows (train_loop_survival(group=True)) --
  epoch 1 and epoch 2 through the cache, an epoch through DevicePrefetcher, and the loop over bags already on the device.
usage: bag_cache_bench.py [gather] [e2e]     env BAG_CACHE_BENCH_ITERS (default 20), BAG_CACHE_BENCH_BAGS (default 8)"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodalfusion_amd import feed, ops
from multimodalfusion_amd.models import MIL_Attention_fc_surv_path

RAGGED = [1000, 20000, 3000, 12000, 1500, 8000, 5000, 2500]
WINDOWS = [("16x1k", [1000] * 16, 1), ("64x1k", [1000] * 64, 1), ("4x10k", [10000] * 4, 1), ("ragged8", RAGGED, 1),
           ("16x(512x4mod)", [512] * 16, 4)]
L = 1024


def timed(fn, iters):
    for _ in range(3):
        fn()
    runs = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) / iters)
    return statistics.median(runs)


def scattered(sizes, nplane, dtype, dev):
    """The window's bags at shuffled, 256-byte aligned places of one arena with gaps between them."""
    item = torch.empty((), dtype=dtype).element_size()
    order = np.random.RandomState(3).permutation(len(sizes) * nplane)
    need = sum(sizes) * nplane * L * item + 8192 * (len(order) + 1)
    arena = torch.empty(need, dtype=torch.uint8, device=dev)
    at, place = 0, {}
    for k in order:
        n = sizes[k % len(sizes)]
        place[k] = arena[at:at + n * L * item].view(dtype).view(n, L)
        place[k].normal_() if dtype == torch.float32 else place[k].copy_(torch.randn(n, L, device=dev))
        at += (n * L * item + 4095) // 4096 * 4096 + 256
    return arena, [[place[m * len(sizes) + g] for g in range(len(sizes))] for m in range(nplane)]


def gather_leg(iters):
    dev = torch.device("cuda", 0)
    for name, sizes, nplane in WINDOWS:
        R, G = sum(sizes), len(sizes)
        _, planes = scattered(sizes, nplane, torch.float32, dev)
        _, planes16 = scattered(sizes, nplane, torch.bfloat16, dev)
        buf = torch.empty(nplane, R, L, device=dev)
        flat = torch.randn(nplane, R, L, device=dev)
        offs = np.concatenate([[0], np.cumsum(sizes)])

        def copies():
            for m in range(nplane):
                for g in range(G):
                    buf[m, offs[g]:offs[g + 1]].copy_(planes[m][g], non_blocking=True)

        t_a = timed(lambda: ops.bag_gather(planes, buf), iters)
        assert all(torch.equal(buf[m], torch.cat(planes[m])) for m in range(nplane))
        t_b = timed(copies, iters)
        t_c = timed(lambda: buf.copy_(flat), iters)
        t_w = timed(lambda: ops.bag_gather(planes16, buf), iters)
        assert all(torch.equal(buf[m], torch.cat(planes16[m]).float()) for m in range(nplane))
        nbytes = nplane * R * L * 4
        print(json.dumps({"window": name, "bags": G, "planes": nplane, "mbytes": round(nbytes / 2 ** 20, 1),
                          "gather_ms": round(t_a, 4), "copies_ms": round(t_b, 4), "contig_ms": round(t_c, 4),
                          "widen_ms": round(t_w, 4), "gather_tb_s": round(2 * nbytes / t_a / 1e9, 3),
                          "contig_tb_s": round(2 * nbytes / t_c / 1e9, 3), "widen_vs_gather": round(t_w / t_a, 3),
                          "gather_lt_copies": t_a < t_b, "yardstick_ok": t_a <= 1.10 * t_c + 0.015}), flush=True)


def host_bags(n_bags, rows):
    out = []
    for i in range(n_bags):
        x = torch.empty(rows, L).pin_memory()
        x.normal_()
        out.append(({"T1": torch.zeros(1, 1)}, x, torch.zeros(1, 4), torch.tensor([i % 4]), np.array([float(10 + i)]),
                    torch.tensor([float(i % 2)])))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def e2e_leg(n_big):
    from multimodalfusion_amd.utils import core_utils
    from multimodalfusion_amd.utils.loss_utils import NLLSurvLoss
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MIL_Attention_fc_surv_path(gate_path=True, model_size_wsi="small", dropout=True, n_classes=4).to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    loss_fn = NLLSurvLoss(alpha=0.2)

    def per_bag(src):
        for _, path, _, label, _, c in src:
            model.nll_step(path, label.to(dev), c.to(dev))

    def grouped(src):
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            core_utils.train_loop_survival(0, model, src, opt, 4, "path", loss_fn=loss_fn, gc=64, group=True)

    for name, rows, n_bags, run in [("50k_one_bag_per_step", 50000, n_big, per_bag), ("64x1k_grouped", 1000, 256, grouped)]:
        host = host_bags(n_bags, rows)
        on_dev = [(r, p.to(dev), g, y.to(dev), t, c.to(dev)) for r, p, g, y, t, c in host]
        run(on_dev)                                       # warm-up: workspaces, the holders' buffer
        e1, e2, pre, res = [], [], [], []
        for _ in range(3):
            cache = feed.ResidentBagCache(host, capacity_bytes=(n_bags * rows * L * 4) * 2 + (64 << 20))
            e1.append(wall(lambda: run(cache)))
            e2.append(wall(lambda: run(cache)))
            stats = cache.stats()
            del cache
            pf = feed.DevicePrefetcher(host)
            pre.append(wall(lambda: run(pf)))
            res.append(wall(lambda: run(on_dev)))
        rate = lambda ts: round(n_bags / statistics.median(ts), 1)
        print(json.dumps({"workload": name, "bags": n_bags, "cache_epoch1_bags_s": rate(e1), "cache_epoch2_bags_s": rate(e2),
                          "prefetcher_bags_s": rate(pre), "resident_loop_bags_s": rate(res),
                          "epoch2_vs_resident": round(statistics.median(res) / statistics.median(e2), 3),
                          "epoch1_vs_prefetcher": round(statistics.median(pre) / statistics.median(e1), 3),
                          "target_epoch2_ge_0.9_resident": statistics.median(res) / statistics.median(e2) >= 0.9,
                          "stats": stats}), flush=True)
        del host, on_dev


if __name__ == "__main__":
    legs = [a for a in sys.argv[1:] if a in ("gather", "e2e")] or ["gather", "e2e"]
    if "gather" in legs:
        gather_leg(int(os.environ.get("BAG_CACHE_BENCH_ITERS", "20")))
    if "e2e" in legs:
        e2e_leg(int(os.environ.get("BAG_CACHE_BENCH_BAGS", "8")))
