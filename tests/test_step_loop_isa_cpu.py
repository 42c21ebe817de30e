"""The step loop of the stride-0 full instantiations (LSO, ev2g_step_wave.h) is peeled: every step but the launch's last runs a body without outputs,
the last one a body with them.  Checked on the device assembly (hipcc cross-compiles gfx950; -DEV2G_PHASE_MARKERS leaves the phase boundaries as
comments), for the headline instantiation <0,0,f64,2> and for PublicPST's <1,1,f64,2>:

  * between the loop header and `PHASE_MARK 0` (the end of phase A) of the body without outputs there is no s_waitcnt on vmcnt: vmcnt counts stores
    as well as loads on gfx950, so a wait there makes every step begin by draining the stores of the step before;
  * the body without outputs holds no store through the observation, mask, reward or done argument (nor the float32 observation's).  The pointers are
    followed from their kernel-argument loads through moves, adds, lane parking and 64-bit address arithmetic to the address operands of every store;
    the body WITH outputs must show such stores (else the tracker would prove nothing).

The static per-phase instruction mix of both bodies is printed (tools/isa_phase_count.py)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {
    "headline <0,0,f64,2>": "_Z14ev2g_step_waveILi0ELi0ELb0ELi2ELi256ELb0ELi1ELi1EE",
    "PublicPST <1,1,f64,2>": "_Z14ev2g_step_waveILi1ELi1ELb0ELi2ELi256ELb0ELi1ELi1EE",
}
# kernel-argument bytes that hold an output pointer: StepIO sits behind the 8-byte parameter-block pointer (ev2g_device.h)
# obs 0x18, reward 0x28, done 0x38, mask 0x48, obs32 0x70
OUT_ARG_BYTES = [(0x18, 0x20), (0x28, 0x30), (0x38, 0x40), (0x48, 0x50), (0x70, 0x78)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from ev2gym_amd import build
    out = str(tmp_path_factory.mktemp("isa") / "markers.s")
    cmd = [build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm", "-disable-machine-licm",
           "-DEV2G_PHASE_MARKERS", "-S", "--cuda-device-only", "-o", out, build.SRC]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return out, open(out).read().split("\n")


def _function(lines, prefix):
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(":")[0].endswith("FusedArgs") and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start:end + 1]


def _marks(fn, k):
    return [i for i, l in enumerate(fn) if l.strip() == f"; PHASE_MARK {k}"]


def _regs(op):
    """The registers an operand names: [('s', 4), ('s', 5)] for s[4:5]."""
    m = re.fullmatch(r"([sv])\[(\d+):(\d+)\]", op)
    if m:
        return [(m.group(1), n) for n in range(int(m.group(2)), int(m.group(3)) + 1)]
    m = re.fullmatch(r"([sv])(\d+)", op)
    return [(m.group(1), int(m.group(2)))] if m else []


def _output_stores(fn):
    """Line indices of the stores whose address comes from an output-pointer argument.  One pass in text order: a register is `out` when it was loaded
    from the output pointers' kernel-argument bytes or computed from an `out` register; any other definition clears it."""
    out, karg, lanes, hits = set(), {("s", 0), ("s", 1)}, set(), []
    two_dst = ("v_mad_u64_u32", "v_mad_i64_i32", "v_add_co_u32", "v_addc_co_u32", "v_sub_co_u32", "v_subb_co_u32", "v_subrev_co_u32", "v_div_scale_f64", "v_div_scale_f32")
    for i, l in enumerate(fn):
        t = l.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        op, _, rest = t.partition(" ")
        ops = [o.strip().split(" ")[0] for o in rest.split(",")] if rest else []
        if op.startswith(("global_store", "flat_store")):
            addr = _regs(ops[0]) + (_regs(ops[2]) if len(ops) > 2 else [])
            if any(r in out for r in addr):
                hits.append(i)
            continue
        if op.startswith(("s_cmp", "s_cbranch", "s_branch", "s_waitcnt", "s_barrier", "s_nop", "s_setprio", "ds_write", "global_atomic", "v_cmpx", "s_bitcmp", "buffer_", "s_endpgm")) or not ops:
            continue
        if op.startswith("v_cmp") and op.endswith("_e32"):
            continue
        dst = _regs(ops[0])
        if op == "v_writelane_b32":   # an SGPR parked in one lane of a VGPR
            key = (ops[0], ops[2])
            (lanes.add if _regs(ops[1]) and _regs(ops[1])[0] in out else lanes.discard)(key)
            continue
        if op == "v_readlane_b32" and (ops[1], ops[2]) in lanes:
            out.update(dst)
            karg.difference_update(dst)
            continue
        if op.startswith("s_load_dword"):
            base, off = _regs(ops[1]), int(ops[2], 0) if re.fullmatch(r"(0x[0-9a-f]+|\d+)", ops[2]) else None
            from_karg = bool(base) and all(r in karg for r in base) and off is not None
            for n, r in enumerate(dst):
                b = (off or 0) + 4 * n
                (out.add if from_karg and any(lo <= b < hi for lo, hi in OUT_ARG_BYTES) else out.discard)(r)
            karg.difference_update(dst)
            continue
        srcs = [r for o in ops[1:] for r in _regs(o)]
        if op in two_dst and len(ops) > 1:
            dst += _regs(ops[1])
        tainted = any(r in out for r in srcs) and not op.startswith(("global_load", "ds_read", "scratch_load"))
        is_karg = op in ("s_mov_b64", "s_mov_b32") and bool(srcs) and all(r in karg for r in srcs)
        for r in dst:
            (out.add if tainted else out.discard)(r)
            (karg.add if is_karg else karg.discard)(r)
    return hits


def _bodies(fn):
    """(first, last) line ranges of the body without outputs -- the loop: its header, or its latch where that is laid out first, up to the second body's
    first mark -- and of the peeled body with them."""
    m7, m5, m0 = _marks(fn, 7), _marks(fn, 5), _marks(fn, 0)
    assert len(m7) == 2 and len(m5) == 2 and len(m0) == 2, ("two step bodies expected", m7, m5, m0)
    header = max(i for i in range(m7[0]) if "Loop Header: Depth=1" in fn[i])
    return (min(header, m5[0]), m7[1]), (m7[1], max(m5)), header, m0[0]


def _mix(name, fn, tmp_path):
    (a0, a1), (b0, b1), _, _ = _bodies(fn)
    for tag, (lo, hi) in (("body without outputs (the loop)", (a0, a1)), ("body with outputs (the launch's last step)", (b0, b1))):
        part = tmp_path / "part.s"
        part.write_text("part:\n" + "\n".join(fn[lo:hi + 1]) + "\n\ts_endpgm\n")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_phase_count.py"), str(part), "part"], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        print(f"{name}, {tag}: static instruction mix per phase\n{p.stdout}")


@pytest.mark.parametrize("name", list(KERNELS))
def test_loop_body_writes_no_output(name, asm, tmp_path):
    path, lines = asm
    fn = _function(lines, KERNELS[name])
    (a0, a1), (b0, b1), header, mark0 = _bodies(fn)
    assert header < mark0 < a1
    hits = _output_stores(fn)
    in_loop, in_last = [i for i in hits if a0 <= i < a1], [i for i in hits if b0 <= i <= b1]
    print(f"{name}: stores through an output argument: {len(in_loop)} in the body without outputs, {len(in_last)} in the body with them")
    for i in in_loop + in_last:
        print(f"    line {i}: {fn[i].strip()}")
    _mix(name, fn, tmp_path)
    assert len(in_last) >= 4, f"{name}: the tracker finds only {len(in_last)} output stores in the body that writes them"
    assert not in_loop, f"{name}: the body without outputs stores through an output argument: {[fn[i].strip() for i in in_loop]}"


@pytest.mark.parametrize("name", list(KERNELS))
def test_loop_top_has_no_wait_on_vmcnt(name, asm):
    """PublicPST's instantiation never had such a wait.  The headline instantiation had two `s_waitcnt vmcnt(0)` there (one in the `tid < 2` branch that
    clears the next step's counters, one in front of the first prefetch).  Their cause was the fast-forward path, not the output stores: the pass left
    the step ahead of phase C's collection point, so along that way round the loop (and along two branches that only the structurised control flow has)
    the step's prefetches were outstanding at the loop header, and the compiler waited in front of the first redefinition of their registers.  The
    decision and the pass now stand behind the collection point: profiles/r27_step_loop.txt."""
    path, lines = asm
    fn = _function(lines, KERNELS[name])
    _, _, header, mark0 = _bodies(fn)
    waits = [fn[i].strip() for i in range(header, mark0) if re.match(r"\s*s_waitcnt\b.*vmcnt", fn[i])]
    print(f"{name}: loop header at line {header}, PHASE_MARK 0 at {mark0}; vmcnt waits between them: {waits}")
    assert not waits, f"{name}: the step loop waits on vmcnt before its first prefetch: {waits}"
