"""CPU guard of the one-call stage-2 step's case table (tests/stage2_step_cases.py): what it must cover, and that float32
arithmetic alone keeps every case within HALF of each bar -- the float32 oracle against the float64 one -- so that a kernel
which misses a bar on the GPU is wrong and not unlucky.  A case that fails here gets another seed in the table's RESEED,
never a wider bar."""
import pytest
import torch

import stage2_step_cases as sc


def test_the_table_covers_what_it_must():
    sc.coverage()
    assert len(sc.CASES) >= 56


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_float32_alone_stays_within_half_of_every_bar(name):
    c = sc.BY_NAME[name]
    ref = sc.oracle(name)
    f32 = sc.oracle(name, torch.float32)
    worst = sc.check(f32, ref, c, factor=0.5, what="fp32 oracle ")
    print(f"{name}: worst error / (bar / 2) = {worst:.3f}")
    if c.special in ("all_censored", "no_pair"):
        assert ref["loss"] == 0.0 and all(float(abs(g).max()) == 0.0 for g in ref["grads"].values()), name
