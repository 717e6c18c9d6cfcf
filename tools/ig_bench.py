"""Integrated-gradients attribution: the fused call (model.integrated_gradients, one mmf_amil_ig or mmf_radio_ig) against the
route without it (infer.integrated_gradients_autograd / radio_integrated_gradients_autograd: one autograd pass per node) on
the same bags, in one process, eval mode, small gated head, 20 Gauss-Legendre nodes.  --head path: the pathology head, b1 ~
N(0, 0.1); --head radio: the radiology head, four modalities of 1024 features, b1 and br ~ N(0, 0.1).  Device-event timing,
warm-up first, median of three runs.  One JSON line per bag size; `ratio` = fused / autograd (required: < 1 everywhere;
<= 0.5 at 50,000 rows of the pathology head and at 150 and 512 rows of the radiology head); `kernels`: the fused call's
per-kernel device time from one traced call; `patch_abs_max_rel_diff` / `inst_abs_max_rel_diff`: the worst difference of
the per-row sums of |attr| between the routes.
--head mm: the multimodal concat head (one mmf_mm_ig), radio_path_omic, small gated stacks, four sequences, an 80-gene omic
vector, every first-layer bias ~ N(0, 0.1); ROWS are (N_p, N_r) pairs; the yardstick is
infer.mm_integrated_gradients_autograd (required: ratio < 1 everywhere); `single_heads_ms`: mmf_amil_ig on the pathology bag
plus mmf_radio_ig on the radiology bags in the same process, each with the classifier's columns of its branch as its head,
and `vs_single_heads` = fused / that sum (reported, not gated); `*_max_rel_diff`: modality_abs, patch_abs, inst_abs.
--head mm --fusion tensor: the tensor-fusion head (one mmf_mm_ig_tensor) on a fusion='tensor' model, every first-layer bias
~ N(0, 0.1) again; the yardstick is the same autograd route on that model (required: ratio < 1 everywhere); `concat_ms`:
mmf_mm_ig on a concat model over the same inputs in the same process, and `tail_ms` = fused - concat, what the fusion tail
costs (reported, not gated).
--head stage2 [--train-type T ...]: the stage-2 multimodal_pretrained (nll, radio_path_omic, n_classes 4, every bias and
BatchNorm statistic drawn) on a cohort of ROWS patients (one mmf_stage2_ig); `autograd_ms`: infer.stage2_integrated_
gradients_autograd over the whole [P x 256] batch; `per_patient_autograd_ms`: the same route one patient at a time, what
the reference's script does (timed on min(P, 8) patients and scaled); required: ratio < 1 everywhere.
usage: ig_bench.py [--head path|radio|mm|stage2] [--fusion concat|tensor] [--train-type T ...] [ROWS ...]   (default rows: 1000 10000 50000, radio 150 512 4096, mm 1000 150
10000 512 50000 512);
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


def timed_alternating(routes):
    """timed() for several (fn, iters) routes at once: every route warmed up, then three rounds that time each route in turn,
    so that a drift of the clocks meets all of them alike; the median per route."""
    for fn, _ in routes:
        for _ in range(2):
            fn()
    runs = [[] for _ in routes]
    for _ in range(3):
        for r, (fn, iters) in zip(runs, routes):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            r.append(a.elapsed_time(b) / iters)
    return [statistics.median(r) for r in runs]


def main_mm(rows, iters, steps, fusion="concat"):
    from multimodalfusion_amd.models.model_mm_attention_mil import MM_MIL_Attention_fc_surv
    from multimodalfusion_amd.models.model_modules import stack_args
    rows = rows or [1000, 150, 10000, 512, 50000, 512]
    if len(rows) % 2:
        sys.exit("--head mm takes (N_p, N_r) pairs")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)

    def make(fusion):
        with torch.no_grad():
            m = MM_MIL_Attention_fc_surv(input_dim=80, fusion=fusion, dropout=False, n_classes=4, mode="radio_path_omic").to(dev).eval()
            for b in (m.attention_net_WSI[0].bias, m.attention_net_radio[0].bias, m.reduce_dim.bias, m.fc_omic[0][0].bias,
                      m.fc_omic[1][0].bias):
                b.normal_(0.0, 0.1)
        return m

    model = make("concat")
    tensor = make("tensor") if fusion == "tensor" else None
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    a, w = (v.astype(np.float32) for v in ops.ig_quadrature("gausslegendre", steps))
    _, cols, _ = model._concat_layout()
    Wk, bk = model.classifier.weight, model.classifier.bias
    gp, sp, _, _ = stack_args(model.attention_net_WSI, False)
    gr, sr, _, _ = stack_args(model.attention_net_radio, False)
    Wk_p, Wk_r = Wk[:, cols["path"]].contiguous(), Wk[:, cols["radio"]].contiguous()
    for Np, Nr in zip(rows[0::2], rows[1::2]):
        feats = {m: torch.randn(Nr, 1024, device=dev, generator=gen) for m in MODS}
        feats["path_features"] = torch.randn(Np, 1024, device=dev, generator=gen)
        feats["genomic_features"] = torch.randn(80, device=dev, generator=gen)
        xs = [feats[m] for m in MODS]

        def fused():
            return model.integrated_gradients(n_steps=steps, **feats)

        def fused_tensor():
            return tensor.integrated_gradients_tensor(n_steps=steps, **feats)

        def autograd():
            return infer.mm_integrated_gradients_autograd(tensor or model, feats, a, w)

        def single_heads():
            with torch.no_grad():
                ops.amil_integrated_gradients(feats["path_features"], sp, Wk_p, bk, gp, a, w)
                ops.radio_integrated_gradients(xs, model.reduce_dim.weight, model.reduce_dim.bias, sr, Wk_r, bk, gr, a, w)

        f, (g, *_) = (fused_tensor if tensor else fused)(), autograd()
        torch.cuda.synchronize()
        ref = {"path": g["path"].abs().sum(1), "radio": g["radio"].abs().sum(2)}
        mod = {b: float(v.abs().sum()) for b, v in g.items()}
        err = {"modality_abs": max(abs(float(f.modality_abs[b]) - mod[b]) / mod[b] for b in mod),
               "patch_abs": float((f.patch_abs - ref["path"]).abs().max() / ref["path"].max()),
               "inst_abs": float((f.inst_abs - ref["radio"]).abs().max() / ref["radio"].max())}
        if tensor:                    # (a) the fused call, (b) the autograd passes on the same model, (c) mmf_mm_ig on a concat model
            t_f, t_a, t_c = timed_alternating([(fused_tensor, iters), (autograd, max(1, iters // 2)), (fused, iters)])
            other = {"concat_ms": round(t_c, 4), "tail_ms": round(t_f - t_c, 4)}
        else:
            t_f, t_a, t_s = timed_alternating([(fused, iters), (autograd, max(1, iters // 2)), (single_heads, iters)])
            other = {"single_heads_ms": round(t_s, 4), "vs_single_heads": round(t_f / t_s, 4)}
        trace = _lib.KernelTrace()
        with trace:
            (fused_tensor if tensor else fused)()
            torch.cuda.synchronize()
        kernels = {k: [c, round(ms, 4)] for k, (c, ms) in sorted(trace.dump().items(), key=lambda kv: -kv[1][1])}
        trace.close()
        ratio = t_f / t_a
        print(json.dumps({"rows": [Np, Nr], "modalities": len(MODS), "n_steps": steps, "fusion": fusion, "fused_ms": round(t_f, 4),
                          "autograd_ms": round(t_a, 4), "ratio": round(ratio, 4), "required": 1.0, "ok": ratio < 1.0, **other,
                          **{k + "_max_rel_diff": float(f"{v:.3e}") for k, v in err.items()},
                          "share": {b: round(float(v), 4) for b, v in f.share.items()}, "kernels": kernels}), flush=True)


STAGE2_TYPES = ["early-fcnn", "late-fcnn", "early-highway", "late-highway", "kronecker"]


def main_stage2(rows, iters, steps, types):
    from multimodalfusion_amd.models.nll_models_pretrained import multimodal_pretrained
    dev = torch.device("cuda", 0)
    a, w = (v.astype(np.float32) for v in ops.ig_quadrature("gausslegendre", steps))
    for tt in types or STAGE2_TYPES:
        torch.manual_seed(0)
        model = multimodal_pretrained(n_classes=4, mode="radio_path_omic", train_type=tt).to(dev).eval()
        with torch.no_grad():
            for k, v in model.state_dict().items():
                if k.endswith("running_var"):
                    v.uniform_(0.5, 1.5)
                elif k.endswith("running_mean") or (v.dim() == 1 and v.dtype.is_floating_point):
                    v.add_(torch.randn_like(v) * 0.1)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        for P in rows or [1, 32, 256]:
            hs = [torch.randn(P, 256, device=dev, generator=gen) for _ in range(3)]
            few = min(P, 8)
            fused = lambda: model.integrated_gradients(*hs, n_steps=steps)
            autograd = lambda: infer.stage2_integrated_gradients_autograd(model, *hs, a, w)

            def per_patient():
                for p in range(few):
                    infer.stage2_integrated_gradients_autograd(model, *[h[p:p + 1] for h in hs], a, w)

            f, g = fused(), autograd()
            torch.cuda.synchronize()
            ref = torch.stack([g[0][n].abs().sum(1) for n in ("radio", "path", "omic")], 1)
            got = torch.stack([f.modality_abs[n] for n in ("radio", "path", "omic")], 1)
            err = float((got - ref).abs().max() / ref.max())
            t_f, t_a, t_p = timed_alternating([(fused, iters), (autograd, max(1, iters // 2)), (per_patient, 1)])
            trace = _lib.KernelTrace()
            with trace:
                fused()
                torch.cuda.synchronize()
            kernels = {k: [c, round(ms, 4)] for k, (c, ms) in sorted(trace.dump().items(), key=lambda kv: -kv[1][1])}
            trace.close()
            print(json.dumps({"train_type": tt, "patients": P, "n_steps": steps, "fused_ms": round(t_f, 4),
                              "autograd_ms": round(t_a, 4), "per_patient_autograd_ms": round(t_p * P / few, 4),
                              "ratio": round(t_f / t_a, 4), "required": 1.0, "ok": t_f < t_a,
                              "modality_abs_max_rel_diff": float(f"{err:.3e}"), "kernels": kernels}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", choices=["path", "radio", "mm", "stage2"], default="path")
    ap.add_argument("--fusion", choices=["concat", "tensor"], default="concat")
    ap.add_argument("--train-type", choices=STAGE2_TYPES, action="append")
    ap.add_argument("rows", nargs="*", type=int)
    args = ap.parse_args()
    if args.fusion == "tensor" and args.head != "mm":
        sys.exit("--fusion tensor goes with --head mm")
    if args.head == "stage2":
        return main_stage2(args.rows, int(os.environ.get("IG_BENCH_ITERS", "5")), int(os.environ.get("IG_BENCH_STEPS", "20")),
                           args.train_type)
    if args.head == "mm":
        return main_mm(args.rows, int(os.environ.get("IG_BENCH_ITERS", "5")), int(os.environ.get("IG_BENCH_STEPS", "20")),
                       args.fusion)
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
