"""Integrated-gradients attribution of the radiology head: the fused call (model.integrated_gradients, one mmf_radio_ig)
against the route without it (infer.radio_integrated_gradients_autograd: one autograd pass per node through reduce_dim and
the stack) on the same bags, in one process, eval mode, gated small head, four modalities of 1024 features, 20
Gauss-Legendre nodes, b1 and br ~ N(0, 0.1).  Device-event timing, warm-up first, median of three runs.  One JSON line per
bag size; `ratio` = fused / autograd (required: < 1 everywhere, <= 0.5 at 150 and 512 rows); `kernels`: the fused call's
per-kernel device time from one traced call; `inst_abs_max_rel_diff`: the worst difference of inst_abs between the routes.
usage: radio_ig_bench.py [ROWS ...]   (default: 150 512 4096);  env IG_BENCH_ITERS (default 5), IG_BENCH_STEPS (default 20)"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodalfusion_amd import _lib, infer, ops
from multimodalfusion_amd.models import MIL_Attention_fc_surv_radio

MODS = ["T1", "T2", "T1Gd", "FLAIR"]


def timed(fn, iters):
    for _ in range(2):
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


def main():
    rows = [int(a) for a in sys.argv[1:]] or [150, 512, 4096]
    iters = int(os.environ.get("IG_BENCH_ITERS", "5"))
    steps = int(os.environ.get("IG_BENCH_STEPS", "20"))
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MIL_Attention_fc_surv_radio(gate_radio=True, dropout=False, n_classes=4, modalities=MODS).to(dev).eval()
    with torch.no_grad():                                       # zero biases would hide the composed bias and the nodes
        model.attention_net_radio[0].bias.normal_(0.0, 0.1)
        model.reduce_dim.bias.normal_(0.0, 0.1)
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    a, w = (v.astype(np.float32) for v in ops.ig_quadrature("gausslegendre", steps))
    for N in rows:
        bags = {m: torch.randn(N, 1024, device=dev, generator=gen) for m in MODS}

        def fused():
            return model.integrated_gradients(n_steps=steps, **bags)

        def autograd():
            return infer.radio_integrated_gradients_autograd(model, bags, a, w)

        f, g = fused(), autograd()
        torch.cuda.synchronize()
        scale = float(g[1].max())
        err = float((f.inst_abs - g[1]).abs().max()) / scale
        t_f, t_a = timed(fused, iters), timed(autograd, max(1, iters // 2))
        trace = _lib.KernelTrace()
        with trace:
            fused()
            torch.cuda.synchronize()
        kernels = {k: [c, round(ms, 4)] for k, (c, ms) in sorted(trace.dump().items(), key=lambda kv: -kv[1][1])}
        trace.close()
        need = 0.5 if N <= 512 else 1.0
        print(json.dumps({"rows": N, "modalities": len(MODS), "n_steps": steps, "fused_ms": round(t_f, 4),
                          "autograd_ms": round(t_a, 4), "ratio": round(t_f / t_a, 4), "required": need,
                          "ok": t_f / t_a <= need if N <= 512 else t_f / t_a < need,
                          "inst_abs_max_rel_diff": float(f"{err:.3e}"), "kernels": kernels}), flush=True)


if __name__ == "__main__":
    main()
