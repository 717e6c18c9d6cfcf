"""Integrated-gradients attribution: the fused call (model.integrated_gradients, one mmf_amil_ig or mmf_radio_ig) against the
route without it (infer.integrated_gradients_autograd / radio_integrated_gradients_autograd: one autograd pass per node) on
the same bags, in one process, eval mode, small gated head, 20 Gauss-Legendre nodes.  --head path: the pathology head, b1 ~
N(0, 0.1); --head radio: the radiology head, four modalities of 1024 features, b1 and br ~ N(0, 0.1).  Device-event timing,
warm-up first, median of three runs.  One JSON line per bag size; `ratio` = fused / autograd (required: < 1 everywhere;
<= 0.5 at 50,000 rows of the pathology head and at 150 and 512 rows of the radiology head); `kernels`: the fused call's
per-kernel device time from one traced call; `patch_abs_max_rel_diff` / `inst_abs_max_rel_diff`: the worst difference of
the per-row sums of |attr| between the routes.
usage: ig_bench.py [--head path|radio] [ROWS ...]   (default rows: 1000 10000 50000, radio 150 512 4096);
env IG_BENCH_ITERS (default 5), IG_BENCH_STEPS (default 20)"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodalfusion_amd import _lib, infer, ops
from multimodalfusion_amd.models import MIL_Attention_fc_surv_path, MIL_Attention_fc_surv_radio

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", choices=["path", "radio"], default="path")
    ap.add_argument("rows", nargs="*", type=int)
    args = ap.parse_args()
    radio = args.head == "radio"
    rows = args.rows or ([150, 512, 4096] if radio else [1000, 10000, 50000])
    iters = int(os.environ.get("IG_BENCH_ITERS", "5"))
    steps = int(os.environ.get("IG_BENCH_STEPS", "20"))
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.no_grad():           # zero biases would give every node the same ReLU pattern and hide the composed bias
        if radio:
            model = MIL_Attention_fc_surv_radio(gate_radio=True, dropout=False, n_classes=4, modalities=MODS).to(dev).eval()
            model.attention_net_radio[0].bias.normal_(0.0, 0.1)
            model.reduce_dim.bias.normal_(0.0, 0.1)
        else:
            model = MIL_Attention_fc_surv_path(gate_path=True, model_size_wsi="small", dropout=False, n_classes=4).to(dev).eval()
            model.attention_net_WSI[0].bias.normal_(0.0, 0.1)
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    a, w = (v.astype(np.float32) for v in ops.ig_quadrature("gausslegendre", steps))
    for N in rows:
        if radio:
            bags = {m: torch.randn(N, 1024, device=dev, generator=gen) for m in MODS}
            need, strict, key = (0.5 if N <= 512 else 1.0), N > 512, "inst_abs"

            def fused():
                return model.integrated_gradients(n_steps=steps, **bags)

            def autograd():
                return infer.radio_integrated_gradients_autograd(model, bags, a, w)
        else:
            x = torch.randn(N, 1024, device=dev, generator=gen)
            need, strict, key = (0.5 if N >= 50000 else 1.0), False, "patch_abs"

            def fused():
                return model.integrated_gradients(x, n_steps=steps)

            def autograd():
                return infer.integrated_gradients_autograd(model, x, a, w)

        f, g = fused(), autograd()
        torch.cuda.synchronize()
        scale = float(g[1].max())
        err = float((getattr(f, key) - g[1]).abs().max()) / scale
        t_f, t_a = timed(fused, iters), timed(autograd, max(1, iters // 2))
        ratio = t_f / t_a
        trace = _lib.KernelTrace()
        with trace:
            fused()
            torch.cuda.synchronize()
        kernels = {k: [c, round(ms, 4)] for k, (c, ms) in sorted(trace.dump().items(), key=lambda kv: -kv[1][1])}
        trace.close()
        print(json.dumps({"rows": N, **({"modalities": len(MODS)} if radio else {}), "n_steps": steps,
                          "fused_ms": round(t_f, 4), "autograd_ms": round(t_a, 4), "ratio": round(ratio, 4),
                          "required": need, "ok": ratio < need if strict else ratio <= need,
                          key + "_max_rel_diff": float(f"{err:.3e}"), "kernels": kernels}), flush=True)


if __name__ == "__main__":
    main()
