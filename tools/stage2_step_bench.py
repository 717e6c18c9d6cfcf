"""Stage-2 training step: the one-call step (model.step: one mmf_stage2_step) against the autograd route of the same commit
(model(...), the loss the loop dispatches, loss.backward(): 20 to 45 launches through the composable entry points) on the
same batch, in one process, train mode, mode radio_path_omic, n_classes 4.  Each family x train type at B = 32, 64, 128 and 256; the
highway types with n_layers 1 and 2; one loss per family (nll: RankingNLLSurvLoss, cox: CoxSurvLoss).  Both routes are
timed as the loop runs them, host issue time included: gradients are cleared with set_to_none before every step (what
optimizer.zero_grad() does), event times arrive as a host array.  Device events around ITERS steps, every route warmed up
first, three rounds that time the routes in turn, the median per route.  One JSON line per row; `ratio` = fused / autograd
(required: < 1 in every row that `step_ok` / `step_ok_forward` = model.step_ok in train / eval mode accepts; the rows it
refuses are the measured exceptions, timed all the same); `launches`: the fused call's kernel launches from one traced call; `forward_ms` /
`forward_autograd_ms`: the validation pass (backward=False against model(...) + loss under no_grad, eval mode).
usage: stage2_step_bench.py [--iters N]      (default 200)"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodalfusion_amd import _lib
from multimodalfusion_amd.models import coxranking_models_pretrained as cm
from multimodalfusion_amd.models import nll_models_pretrained as nm
from multimodalfusion_amd.utils.core_utils_pretrained import _loss
from multimodalfusion_amd.utils.loss_utils import CoxSurvLoss, RankingNLLSurvLoss

DEV = torch.device("cuda")


def timed_alternating(routes, iters):
    for fn in routes:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    runs = [[] for _ in routes]
    for _ in range(3):
        for r, fn in zip(runs, routes):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            r.append(a.elapsed_time(b) / iters)
    return [statistics.median(r) for r in runs]


def row(family, tt, B, n_layers, iters):
    torch.manual_seed(0)
    K = 4 if family == "nll" else 1
    model = (nm if family == "nll" else cm).multimodal_pretrained(n_classes=K, mode="radio_path_omic", train_type=tt,
                                                                   n_layers=n_layers).to(DEV)
    loss_fn = RankingNLLSurvLoss() if family == "nll" else CoxSurvLoss()
    g = torch.Generator().manual_seed(1)
    hs = [torch.randn(B, 256, generator=g).to(DEV) for _ in range(3)]
    Y = torch.randint(0, 4, (B,), generator=g).to(DEV)
    t = (torch.randint(0, 40, (B,), generator=g).double() / 2).numpy()
    c = (torch.rand(B, generator=g) < 0.4).float().to(DEV)
    params = list(model.parameters())

    def clear():
        for p in params:
            p.grad = None

    def fused():
        clear()
        model.step(*hs, loss_fn, label=Y, event_time=t, c=c)

    def autograd():
        clear()
        risk, hazards, S = model(h_radio=hs[0], h_path=hs[1], h_omic=hs[2])
        _loss(loss_fn, risk, hazards, S, Y, t, c, DEV).backward()

    def fused_fwd():
        model.step(*hs, loss_fn, label=Y, event_time=t, c=c, backward=False)

    def autograd_fwd():
        with torch.no_grad():
            risk, hazards, S = model(h_radio=hs[0], h_path=hs[1], h_omic=hs[2])
            _loss(loss_fn, risk, hazards, S, Y, t, c, DEV)

    model.train()
    ok_train = bool(model.step_ok(*hs, loss_fn))
    f_ms, a_ms = timed_alternating([fused, autograd], iters)
    tr = _lib.KernelTrace(256)
    with tr:
        fused()
    torch.cuda.synchronize()
    launches = sum(n for n, _ in tr.dump().values())
    tr.close()
    model.eval()
    ok_eval = bool(model.step_ok(*hs, loss_fn))
    ff_ms, af_ms = timed_alternating([fused_fwd, autograd_fwd], iters)
    return dict(family=family, train_type=tt, B=B, n_layers=n_layers, loss=type(loss_fn).__name__, fused_ms=round(f_ms, 4),
                autograd_ms=round(a_ms, 4), ratio=round(f_ms / a_ms, 3), launches=launches, forward_ms=round(ff_ms, 4),
                forward_autograd_ms=round(af_ms, 4), forward_ratio=round(ff_ms / af_ms, 3), step_ok=ok_train,
                step_ok_forward=ok_eval)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stage2_step_bench.py needs the GPU: there is no CPU path")
    worst = 0.0
    for family in ("nll", "cox"):
        for tt in ("early-fcnn", "late-fcnn", "early-highway", "late-highway"):
            for n_layers in ((1, 2) if "highway" in tt else (1,)):
                for B in (32, 64, 128, 256):
                    r = row(family, tt, B, n_layers, a.iters)
                    worst = max(worst, r["ratio"] if r["step_ok"] else 0.0, r["forward_ratio"] if r["step_ok_forward"] else 0.0)
                    print(json.dumps(r), flush=True)
    print(json.dumps(dict(worst_ratio_where_step_ok=worst, every_row_step_ok_takes_is_faster=worst < 1.0)), flush=True)


if __name__ == "__main__":
    main()
