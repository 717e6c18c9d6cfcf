"""Bags at the row caps of the attention stack, kept small: cases, inputs and float64 oracle of tests/test_gpu_row_caps.py
(helper module, not collected by pytest).  tests/test_cap_cases_cpu.py checks the conditions below on these very arrays.

Inputs.  A bag at the cap is a small base bag repeated: row i = base[i mod n0], gathered on the device.  Softmax pooling
sees the repeated bag as the base bag with row multiplicities m_j = #{i < N : i mod n0 = j}:

  scores     row-local: row i's score is base row (i mod n0)'s;
  pooled     sum_i e^{s_i} h_i / sum_i e^{s_i} = sum_j m_j e^{s_j} h_j / sum_j m_j e^{s_j}: M, the hazards, the loss and --
             as the same function of the parameters -- every parameter gradient are those of the base bag with log m_j
             added to the scores before the softmax.  Uniform m_j cancel: the plain base bag.

Caps with divisors give uniform multiplicities (N = n0 * m); n0 is above 256 rows and no multiple of 16.  2^19 - 1 =
524,287, the cap of every fp32 stack whose widest row is 1024, is prime: those cases repeat 337 rows 1555 times and the
first 252 once more.

Oracle.  periodic_oracle: float64, from the pieces of oracle/torch_port.py (_lin, attn_net, surv_head, nll_loss) cut the
way tests/ig_cases.py _dh cuts them, with log m_j in the softmax; with uniform multiplicities it is oracle.cases.run_path
on the base bag to 1e-12 (tests/test_cap_cases_cpu.py).  bf16 storage: oracle/bf16_port.path_step_bf16, unchanged, on the
base bag -- uniform multiplicities only.

No ReLU excuses.  A hidden unit whose float64 pre-activation lies within the projection's summation bound of zero,
|u| <= (L / 2 + 8) * 2^-24 * (sum_l |x_l W1_jl| + |b1_j|) (tests/ig_cases.py), may land on the other side of the ReLU in
fp32.  Every row of a base bag with such a unit is redrawn from the seeded generator until no unit of the bag is flagged, so
that no comparison skips or loosens anything for a kink."""
import collections
import functools

import numpy as np
import torch

from oracle import bf16_port, cases
from oracle import inputs as gen
from oracle import torch_port as tp

U = 2.0 ** -24
MAX_ROUNDS = 6          # redraw rounds any base bag may need (tests/test_cap_cases_cpu.py pins each case's count)
PRE = "attention_net_WSI"

# chain: f32 / bf16 (mmf_amil_nll_step), group (mmf_amil_nll_step_group and mmf_amil_infer_group), scorer (mmf_attn_net_*),
# train (scores of a train-mode step).  gemm: MMF_GEMM_F32 / MMF_GEMM_BF16X3.  periods: the bags of a window, in base bags.
Case = collections.namedtuple("Case", "name chain size gated N n0 gemm periods seed why")

SMALL = (1024, 256, 256)


def _c(name, chain, size, gated, N, n0, gemm=0, periods=(), seed=0, why=""):
    return Case(name, chain, size, gated, N, n0, gemm, periods, seed or 7000 + 13 * len(name) + size[0] + size[2], why)


F32 = [
    _c("f32_32_256_128_ungated", "f32", (32, 256, 128), False, 2**21 - 1, 337, why="h and du end 1 KiB below 2 GiB"),
    _c("f32_128_1024_128_gated", "f32", (128, 1024, 128), True, 2**19 - 1, 337, why="the H-wide operands at the corrected cap"),
    _c("f32_small_gated", "f32", SMALL, True, 2**19 - 1, 337, why="the shipped small head: a 2 GiB bag, wide tiles, 256-wide split-K TN"),
    _c("f32_small_gated_bf16x3", "f32", SMALL, True, 2**19 - 1, 337, gemm=1, why="the same on the split-operand loaders"),
    _c("f32_160_512_640_gated", "f32", (160, 512, 640), True, 419430, 341, why="where 2 D sets the cap"),
]
BF16 = [
    _c("bf16_small_gated", "bf16", SMALL, True, 2**20 - 1, 341, why="the shipped small head in bf16 storage, dh2"),
    _c("bf16_64_512_384_ungated", "bf16", (64, 512, 384), False, 1398101, 683, why="the unfused route, ungated"),
    _c("bf16_64_1024_128_gated", "bf16", (64, 1024, 128), True, 2**20 - 1, 341, why="the H-wide operands at the corrected bf16 cap"),
]
GROUP = _c("group_96_256_128_ungated", "group", (96, 256, 128), False, 2**21 - 1, 337, periods=(1, 700, 5000, 522),
           why="a window of sum N at the cap: one bag of a single period, one with most of the rows")
SCORER = _c("scorer_256_128_gated", "scorer", (256, 256, 128), True, 2**21 - 1, 337, why="the stand-alone scorer, x [N x H] ending 1 KiB below 2 GiB")
TRAIN = _c("train_32_256_128_ungated", "train", (32, 256, 128), False, 2**21 - 1, 337, why="mask indices up to N * H = 2^29 at p_h = p_att = 0.25")
CASES = F32 + BF16 + [GROUP, SCORER, TRAIN]
BY_NAME = {c.name: c for c in CASES}
WEIGHTED = 2**19 - 1                                  # prime: the one N with two different multiplicities
K, ALPHA, BIAS_STD = 4, 0.15, 0.05
MASK_SEED, P_DROP = 977, 0.25
EDGE_ROWS = 512                                       # the train case compares the first and the last EDGE_ROWS rows


def meta(c, n=None):
    """The oracle.cases record of the case's base bag (its raw draw: base_bag redraws the flagged rows)."""
    n = c.n0 if n is None else n
    return dict(N=n, gated=c.gated, size=c.size, K=K, dropout=c.chain == "train", y=c.n0 % 4, c=c.n0 % 2, alpha=ALPHA,
                bias_std=BIAS_STD, train=False, seed=c.seed, x_seed=c.seed + 1000, mask_seed=MASK_SEED)


def multiplicities(N, n0):
    """m_j = #{i < N : i mod n0 = j}."""
    return np.full(n0, N // n0, np.int64) + (np.arange(n0) < N % n0)


def flagged_units(sd, x):
    """[n x H] bool: float64 pre-activations within the projection's summation bound of zero."""
    W1, b1 = np.asarray(sd[PRE + ".0.weight"], np.float64), np.asarray(sd[PRE + ".0.bias"], np.float64)
    x = np.asarray(x, np.float64)
    u = x @ W1.T + b1
    return np.abs(u) <= (x.shape[1] // 2 + 8) * U * (np.abs(x) @ np.abs(W1).T + np.abs(b1))


@functools.lru_cache(maxsize=None)
def base_bag(name):
    """(state dict, base bag [n0 x L] fp32, redraw rounds).  Round k replaces every row that still holds a flagged unit by
    the same row of the generator's draw under seed x_seed + k."""
    c = BY_NAME[name]
    m = meta(c)
    sd, x, _ = cases.path_inputs(m)
    if c.chain == "scorer":                             # no projection in front: the bag is the scorer's input, nothing to flag
        return sd, x[:, :c.size[1]].copy(), 0
    x = x.copy()
    rounds = 0
    while True:
        rows = np.nonzero(flagged_units(sd, x).any(axis=1))[0]
        if rows.size == 0:
            break
        rounds += 1
        assert rounds <= MAX_ROUNDS, (name, rounds)
        x[rows] = gen.bag(m["x_seed"] + rounds, c.n0, dim=c.size[0])[rows]
    x.setflags(write=False)
    return sd, x, rounds


def periodic_oracle(sd, base, mult, y, c, alpha, gated, dropout=False):
    """One forward + nll_surv + backward, in float64, of the bag that holds base row j mult[j] times: path_forward's
    arithmetic (oracle/torch_port.py) cut at the softmax, where log mult is added.  Returns path_step's record (A_raw: the
    base rows' scores)."""
    sdt = tp.to_torch(sd, torch.float64)
    x = torch.as_tensor(np.array(base)).double()
    m = torch.as_tensor(np.asarray(mult, np.float64))
    u = tp._lin(sdt, PRE + ".0", x)
    h = torch.relu(u)
    A, _ = tp.attn_net(sdt, PRE + ".3", h, gated, dropout, None)
    A_raw = A.T
    w = torch.softmax(A_raw + torch.log(m)[None, :], dim=1)         # w_j = m_j e^{s_j} / sum_k m_k e^{s_k}
    M = w @ h
    hz, S, Yh = tp.surv_head(tp._lin(sdt, "classifier", M))
    loss = tp.nll_loss(hz, S, torch.tensor([int(y)]), torch.tensor([float(c)]), alpha=alpha)
    g = tp.grads_of(loss, sdt)
    out = {k: v.detach().numpy() for k, v in dict(hazards=hz, S=S, Y_hat=Yh, A_raw=A_raw, M=M, loss=loss).items()}
    out["grads"] = {k: v.detach().numpy() for k, v in g.items()}
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The float64 oracle of a case (f32, group, train: periodic_oracle; group: per bag g with labels y = g % K, c = g % 2),
    computed once and left unchanged."""
    c = BY_NAME[name]
    sd, x, _ = base_bag(name)
    m = meta(c)
    if c.chain == "group":
        mult = np.ones(c.n0)
        return [periodic_oracle(sd, x, mult, g % K, g % 2, ALPHA, c.gated) for g in range(len(c.periods))]
    return periodic_oracle(sd, x, multiplicities(c.N, c.n0), m["y"], m["c"], ALPHA, c.gated, m["dropout"])


def xq(name):
    """The base bag rounded to bf16 (as float64)."""
    return bf16_port.rb(bf16_port._t(np.array(base_bag(name)[1]))).numpy()


@functools.lru_cache(maxsize=None)
def oracle_bf16(name):
    c = BY_NAME[name]
    assert c.N % c.n0 == 0, "the bf16 oracle takes the plain base bag: uniform multiplicities only"
    sd, _, _ = base_bag(name)
    m = meta(c)
    return bf16_port.path_step_bf16(sd, xq(name), m["y"], m["c"], ALPHA, gated=c.gated, dropout=False, masks=None)


@functools.lru_cache(maxsize=None)
def scorer_oracle(name):
    """Scores, parameter gradients and the base rows' input gradients of the scorer under gA: row i's gA is gA_base[i mod n0],
    so a parameter gradient is sum_j m_j (base row j's term) -- gA_base * m on the base bag -- and row i's dx is base row
    (i mod n0)'s under gA_base."""
    c = BY_NAME[name]
    sd, x, _ = base_bag(name)
    gA = gen.normal(c.seed + 5, (c.n0, 1), stream=3).astype(np.float64)
    sdt = tp.to_torch({k: v for k, v in sd.items() if k.startswith(PRE + ".3")}, torch.float64)
    xt = torch.as_tensor(np.array(x)).double().requires_grad_(True)
    A, _ = tp.attn_net(sdt, PRE + ".3", xt, c.gated, False, None)
    mult = torch.as_tensor(multiplicities(c.N, c.n0).astype(np.float64))[:, None]
    gp = torch.autograd.grad(A, list(sdt.values()), torch.as_tensor(gA) * mult, retain_graph=True)
    (gx,) = torch.autograd.grad(A, xt, torch.as_tensor(gA))
    return dict(A=A.detach().numpy().reshape(-1), gA=gA.reshape(-1), dx=gx.numpy(),
                grads={k: v.numpy() for k, v in zip(sdt, gp)})


def train_scores(name, rows):
    """float64 scores of the given rows (true indices) of the train case under the hash masks of MASK_SEED: h's mask at
    element row * H + col (site 0), a's at row * D + col (site 1).  Scores are row-local."""
    from multimodalfusion_amd import _lib
    c = BY_NAME[name]
    l = _lib.lib()
    sd, x, _ = base_bag(name)
    L, H, D = c.size
    rows = np.asarray(rows, np.int64)

    def mask(site, width):
        keep = np.array([[l.mmf_dropout_keep_host(MASK_SEED, site, int((r * width + j) & 0xFFFFFFFF), P_DROP)
                          for j in range(width)] for r in rows], np.float64)
        return torch.as_tensor(keep / (1.0 - P_DROP))
    sdt = tp.to_torch(sd, torch.float64, False)
    h = torch.relu(tp._lin(sdt, PRE + ".0", torch.as_tensor(x[rows % c.n0]).double())) * mask(0, H)
    masks = {"a": mask(1, D)}
    if c.gated:
        masks["b"] = mask(2, D)
    A, _ = tp.attn_net(sdt, PRE + ".3", h, c.gated, True, masks)
    return A.numpy().reshape(-1)
