"""CPU: tools/isa_check.py (the static guard `build.py --keep-temps` runs on the hand-synchronised bf16 kernels) must catch what
it is there to catch.  Synthetic ISA: a kernel whose hand-issued load is followed by a register copy of its destination before
the hand-placed wait, one whose wait is not covered by enough younger VM operations, one with scratch and packed fp32, and a
clean one; device-scope handoffs (rule 4) that are and are not waited for before their atomic.  And rule 4 on the device
assembly of the two units that hand values across workgroups: the omic step's grid barrier, the K-split ticket."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_check  # noqa: E402


def _kernel(name, body, scratch=0):
    return f"""
\t.text
{name}:
{body}
\ts_endpgm
.Lfunc_end_{name}:
\t.amdhsa_kernel {name}
\t\t.amdhsa_private_segment_fixed_size {scratch}
\t.end_amdhsa_kernel
"""


LOAD = "\t;;#ASMSTART\n\tbuffer_load_dwordx4 v[10:13], v1, s[4:7], s8 offen offset:0\n\t;;#ASMEND\n"
DMA = "\tbuffer_load_dwordx4 v20, s[12:15], s9 offen lds\n"
WAIT4 = "\t;;#ASMSTART\n\ts_waitcnt vmcnt(4)\n\t;;#ASMEND\n"


def _check(tmp_path, text):
    p = tmp_path / "k.s"
    p.write_text(text)
    return isa_check.check_file(str(p), verbose=False)


def test_clean_kernel_passes(tmp_path):
    body = LOAD + DMA * 4 + "\tv_mfma_f32_32x32x16_bf16 v[30:45], v[50:53], v[54:57], v[30:45]\n" + WAIT4 + "\tv_mov_b32_e32 v2, v10\n"
    assert _check(tmp_path, _kernel("_ZN3mmf27amil_fwd_fused2_bf16_kernelILb1EEEv", body)) == []


def test_copy_of_an_unanswered_load_is_flagged(tmp_path):
    body = LOAD + DMA * 4 + "\tv_mov_b32_e32 v99, v11\n" + WAIT4
    bad = _check(tmp_path, _kernel("_ZN3mmf27amil_fwd_fused2_bf16_kernelILb1EEEv", body))
    assert len(bad) == 1 and "in flight" in bad[0] and "v_mov_b32_e32 v99, v11" in bad[0]


def test_uncovered_wait_branch_scratch_and_packed_ops_are_flagged(tmp_path):
    body = LOAD + DMA * 2 + WAIT4                       # vmcnt(4) behind only two younger VM operations
    bad = _check(tmp_path, _kernel("_ZN3mmf27amil_fwd_fused2_bf16_kernelILb1EEEv", body))
    assert any("younger VM operations" in b for b in bad)
    body = LOAD + "\ts_cbranch_scc1 .LBB0_3\n" + DMA * 4 + WAIT4
    bad = _check(tmp_path, _kernel("_ZN3mmf27amil_fwd_fused2_bf16_kernelILb1EEEv", body))
    assert any("branch between" in b for b in bad)
    body = "\tscratch_store_dword off, v3, s0\n\tv_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[2:3]\n"
    bad = _check(tmp_path, _kernel("_ZN3mmf27amil_fwd_fused2_bf16_kernelILb0EEEv", body, scratch=16))
    assert any("scratch" in b for b in bad) and any("packed-fp32" in b for b in bad)
    # other kernels may hold packed fp32 and scratch: the rules are for the two hand-scheduled units
    assert _check(tmp_path, _kernel("_ZN3mmf13reduce_kernelENS_12ReduceParamsE", body, scratch=16)) == []


# rule 4: a device-scope (sc1) store must have completed (s_waitcnt vmcnt(0)) before the kernel takes an atomic ticket
DEV_STORE = "\tglobal_store_dword v[6:7], v2, off sc1\n"
PLAIN_STORE = "\tglobal_store_dword v[6:7], v2, off\n"
TICKET = "\tglobal_atomic_add v2, v3, s[52:53]\n"
PREFETCH = "\tglobal_load_dword v40, v[8:9], off\n" * 3
GRID = "_ZN3mmf22maxnet_cox_step_kernelILi32EEEvNS_16MaxnetStepParamsE"


def _handoffs(tmp_path, body):
    p = tmp_path / "k.s"
    p.write_text(_kernel(GRID, body))
    return isa_check.check_handoff_file(str(p), verbose=False), isa_check.check_file(str(p), verbose=False)


def test_handoff_across_a_bare_barrier_is_flagged(tmp_path):
    for bad in _handoffs(tmp_path, DEV_STORE + "\ts_barrier\n" + PREFETCH + TICKET):
        assert len(bad) == 1 and GRID in bad[0]
        assert "line 4" in bad[0] and "line 9" in bad[0]          # the store's line and the atomic's line of k.s


def test_handoff_behind_vmcnt0_is_clean(tmp_path):
    for bad in _handoffs(tmp_path, DEV_STORE + "\ts_waitcnt vmcnt(0)\n\ts_barrier\n" + PREFETCH + TICKET):
        assert bad == []
    for bad in _handoffs(tmp_path, DEV_STORE + "\ts_waitcnt vmcnt(0) lgkmcnt(0)\n" + TICKET):
        assert bad == []


def test_partial_vmcnt_wait_does_not_close_the_handoff(tmp_path):
    for bad in _handoffs(tmp_path, DEV_STORE + PREFETCH + "\ts_waitcnt vmcnt(2)\n\ts_barrier\n" + TICKET):
        assert len(bad) == 1 and "atomic" in bad[0]


def test_plain_store_before_an_atomic_is_not_flagged(tmp_path):
    for bad in _handoffs(tmp_path, PLAIN_STORE + "\ts_barrier\n" + TICKET):
        assert bad == []
    # a store after the atomic opens a handoff no atomic follows
    for bad in _handoffs(tmp_path, TICKET + DEV_STORE + "\ts_endpgm\n"):
        assert bad == []


# rule 4 on the real sources: the kernels that hand values across workgroups through device-scope stores and a ticket
def _device_asm(tmp_path, unit, reuse):
    """gfx950 assembly of csrc/<unit>.hip with the build's own flags: a device-only compile into tmp_path, or (`reuse`) the
    -save-temps output of `build.py --keep-temps` when that is newer than the source and its headers."""
    import shutil
    import subprocess
    from multimodalfusion_amd import build
    src = os.path.join(build.CSRC, unit + ".hip")
    kept = os.path.join(build.OBJ, unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    if reuse and not build._stale(kept, [src] + [os.path.join(build.CSRC, h) for h in build.HEADERS]):
        return kept
    hipcc = build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    out = str(tmp_path / (unit + ".s"))
    r = subprocess.run([hipcc] + build.FLAGS + build.FILE_FLAGS.get(unit + ".hip", []) +
                       ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _handoff_census(path):
    ks = isa_check.kernels(open(path).read())
    return {n: (sum(1 for _, t, _ in b if isa_check.DEV_STORE.match(t)), sum(1 for _, t, _ in b if isa_check.ATOMIC.match(t)))
            for n, b in ks.items()}


def test_omic_step_orders_its_risk_handoff(tmp_path):
    """mmf_maxnet_cox_step: each workgroup stores its rows' risks at device scope and takes grid barrier 1's ticket; every
    workgroup reads every risk behind it.  Both instantiations (32 and 64 workgroups) must wait for the stores first."""
    path = _device_asm(tmp_path, "mmf_maxnet", reuse=False)      # ~6 s
    census = _handoff_census(path)
    steps = {n: c for n, c in census.items() if "maxnet_cox_step_kernel" in n}
    assert any("ILi32E" in n for n in steps) and any("ILi64E" in n for n in steps), sorted(census)
    for n, (stores, atomics) in steps.items():
        assert stores >= 1 and atomics >= 1, (n, stores, atomics)
    bad = isa_check.check_handoff_file(path, verbose=False)
    assert not bad, "\n".join(bad)


def test_ksplit_ticket_orders_its_partials(tmp_path):
    """mmf_amil_fwd: the K-split projection publishes its partial tiles at device scope before the ticket that lets the
    last slice reduce them (ksplit_publish)."""
    path = _device_asm(tmp_path, "mmf_amil_fwd", reuse=True)   # ~2.5 min to compile
    census = _handoff_census(path)
    both = [n for n, (s, a) in census.items() if s >= 1 and a >= 1]
    assert both, "no kernel of mmf_amil_fwd holds both a device-scope store and an atomic"
    bad = isa_check.check_handoff_file(path, verbose=False)
    assert not bad, "\n".join(bad)
