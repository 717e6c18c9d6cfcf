"""The radiology head's grouped training step (MIL_Attention_fc_surv_radio.nll_step_group, four modalities) against the
same bags one nll_step at a time and against ONE radio bag of the window's total rows, in one process, train mode.
Device-event timing, warm-up first, median of three runs.  One JSON line per case.
usage: radio_group_bench.py [--grouped-only] [CASE ...]   CASE = comma-separated bag sizes, e.g. 16x512 or 96,600,250
       (default: 16x512, a ragged 8-bag window of 96-600 rows, 64x150);  env GROUP_BENCH_ITERS (default 20)
       --grouped-only: time the grouped leg alone (a kernel trace of the run then shows the grouped chain only)"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from group_bench import parse, timed
from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio

MODS = ["T1", "T2", "T1Gd", "FLAIR"]
RAGGED = [96, 600, 250, 420, 128, 512, 333, 180]


def main():
    args = sys.argv[1:]
    grouped_only = "--grouped-only" in args
    cases = [parse(a) for a in args if a != "--grouped-only"] or [[512] * 16, RAGGED, [150] * 64]
    iters = int(os.environ.get("GROUP_BENCH_ITERS", "20"))
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MIL_Attention_fc_surv_radio(radio_fusion="concat", gate_radio=True, dropout=True, n_classes=4,
                                        modalities=MODS).to(dev).train()
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    for sizes in cases:
        G, R = len(sizes), sum(sizes)
        x = torch.randn(len(MODS), R, 1024, device=dev, generator=gen)
        bags = [dict(zip(MODS, parts)) for parts in zip(*[torch.split(x[m], sizes) for m in range(len(MODS))])]
        one = dict(zip(MODS, x.unbind(0)))              # one bag of R rows
        Y = torch.tensor([g % 4 for g in range(G)], device=dev)
        c = torch.tensor([float(g % 2) for g in range(G)], device=dev)

        def grouped():
            model.nll_step_group((x, sizes), Y, c, loss_scale=1.0 / G)

        def sequential():
            for g in range(G):
                model.nll_step(Y[g:g + 1], c[g:g + 1], loss_scale=1.0 / G, **bags[g])

        def one_bag():
            model.nll_step(Y[:1], c[:1], **one)

        t_g = timed(grouped, iters)
        if grouped_only:
            print(json.dumps({"bags": G, "rows": R, "grouped_ms_window": round(t_g, 4),
                              "grouped_ms_per_bag": round(t_g / G, 4)}), flush=True)
            continue
        t_s, t_1 = timed(sequential, max(2, iters // 4)), timed(one_bag, iters)
        print(json.dumps({"bags": G, "rows": R, "sizes": sizes if len(set(sizes)) > 1 else f"{G}x{sizes[0]}",
                          "grouped_ms_window": round(t_g, 4), "grouped_ms_per_bag": round(t_g / G, 4),
                          "sequential_ms_window": round(t_s, 4), "sequential_ms_per_bag": round(t_s / G, 4),
                          "one_bag_of_R_ms": round(t_1, 4),
                          "grouped_vs_one_bag": round(t_g / t_1, 3),
                          "yardstick_ok": t_g <= 1.10 * t_1 + 0.015}), flush=True)
        for p in model.parameters():
            p.grad = None


if __name__ == "__main__":
    main()
