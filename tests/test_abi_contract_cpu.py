"""The arena harness of tests/abi_arena.py without a GPU: its table against the header, the layout of every GPU case (alignment residues
and guard sizes), the harness on fake entries written in numpy (one that overruns y, one that reads a poisoned scale byte, one that
needs a zeroed workspace, one that is correct), the conditions the limit cases of test_abi_limits_gpu.py rest on, and the workspace size
functions at and just past the header's maxima."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import abi_arena as A  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "bie_hip.h")


def launching_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(?:int|size_t)\s+(bie_(?:ternary|mxfp)\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return sorted(name for name, args in protos if re.search(r"\bvoid\s*\*\s*stream\b", args))


def test_every_launching_entry_of_the_header_is_in_the_table():
    names = launching_prototypes()
    assert len(names) >= 40 and "bie_mxfp8_quantize_act" in names and "bie_ternary_pack" in names
    table = set(A.entries())
    assert not table & set(A.EXCLUDED)
    for n in names:
        assert n in table or (n in A.EXCLUDED and len(A.EXCLUDED[n]) > 20), f"{n} is neither in the table nor excluded with a reason"
    assert (table | set(A.EXCLUDED)) <= set(names), sorted((table | set(A.EXCLUDED)) - set(names))


def assert_layout(case):
    lay, total = A.layout(case.ops)
    prev_end, prev_guard = 0, 0
    for o in case.ops:
        off, n = lay[o.name]
        assert n == o.nbytes and o.guard >= A.GUARD_MIN and o.guard >= 128 * o.row_bytes
        assert off % (2 * o.align) == o.align, (case.id, o.name, off, o.align)  # exactly the stated alignment; odd for a 1-byte operand
        assert off - prev_end >= prev_guard + o.guard, (case.id, o.name)         # the guards of two neighbours do not overlap
        prev_end, prev_guard = off + n, o.guard
    assert total - prev_end >= prev_guard and total % A.TIGHT_ALIGN == 0
    tight, _ = A.layout(case.ops, exact=False)
    assert all(off % A.TIGHT_ALIGN == 0 for off, _ in tight.values())


@pytest.mark.parametrize("entry", sorted(A.entries()))
def test_layout_of_every_gpu_case(entry):
    cases = A.cases(entry)
    assert cases
    for c in cases:
        assert c.entry == entry
        assert_layout(c)
        if c.ws is not None:  # the workspace is exactly what the size function says, and that is not 0 for a shape the entry takes
            ws = [o for o in c.ops if o.kind == "ws"]
            assert len(ws) == 1 and ws[0].nbytes == getattr(A.lib(), c.ws[0])(*c.ws[1]) > 0, c.id
        assert sum(o.kind == "out" for o in c.ops) >= 1


def test_layout_of_the_limit_cases_that_run_in_the_arena():
    """E = 1024 and S = 32 of tests/test_abi_limits_gpu.py."""
    for form in (0, 1):
        T, S, idx = A.routing_e1024(form)
        for fam in A.FAMS:
            c = A.experts_case(fam, T, S, A.EMAX, 17, 32, torch.float16, True, 0, form, idx=idx)
            assert_layout(c)
            assert c.ws is None or [o.nbytes for o in c.ops if o.kind == "ws"] == [getattr(A.lib(), c.ws[0])(*c.ws[1])]
            assert_layout(A.experts_case(fam, 3, A.SMAX, 3, 17, 32, torch.bfloat16, True, form, form))
    T, S, idx = A.routing_e1024(1)
    for fmt in ("fp4", "fp6"):
        assert_layout(A.moe_grad_case(fmt, T, S, A.EMAX, 17, 32, torch.float16, 1, idx=idx))
        assert_layout(A.moe_grad_case(fmt, 3, A.SMAX, 3, 17, 32, torch.float16, 0))


def test_ternary_cases_select_the_forms_they_are_listed_under():
    L = A.lib()
    for form, geoms in ((1, A.CONV_FORM1), (2, A.CONV_FORM2)):
        for B, C, H, W, OC, k, st, pad in geoms:
            assert L.bie_ternary_conv2d_form(B, C, H, W, OC, k, st, pad, 1) == form
    B, C, H, W, OC, k, st, pad = A.CONV_FORM1[0]
    assert L.bie_ternary_conv2d_form(B, C - 32, H, W, OC, k, st, pad, 1) != 1       # no smaller C takes the VALU form
    B, C, H, W, OC, k, st, pad = A.CONV_FORM2[0]
    assert L.bie_ternary_conv2d_form(B, C - 32, H, W, OC, k, st, pad, 1) == 0       # nor the matrix-pipe form
    E = A.entries()
    assert all(L.bie_ternary_linear_fused_ok(M, N, K) for M, N, K, _, _ in E["bie_ternary_linear_fused"][1])
    assert any(N > 16384 for _, N, _, _, _ in E["bie_ternary_linear_fused"][1])
    fused = E["bie_ternary_a8_linear_fused"][1]
    assert all(L.bie_ternary_a8_fused_ok(M, N, K) for M, N, K, *_ in fused)
    assert {M for M, *_ in fused} >= {1, 2, 3, 4, 8} and any(N > 16384 for _, N, *_ in fused)
    gemm = E["bie_ternary_a8_linear_gemm"][1]
    assert any(-(-M // 256) * -(-N // 256) >= 192 for M, N, *_ in gemm) and sum(g[6] > g[2] for g in gemm) >= 3  # cases with pad bytes K .. ldq - 1


def test_image_holds_poison_around_inputs_and_a_valid_expert_around_idx():
    c = A.experts_case("mxfp4", 5, 2, 3, 17, 32, torch.float16, True, 0, 1)
    lay, total = A.layout(c.ops)
    img = A.image(c.ops, lay, total, 0x00)
    for o in c.ops:
        off, n = lay[o.name]
        before, after = img[off - o.guard:off], img[off + n:off + n + o.guard]
        if o.name == "idx":
            words = np.concatenate([before, after]).view(np.int32)
            assert (words == 2).all()  # E - 1: in range, so an over-read makes pairs, never a wild expert
        elif o.kind == "in":
            assert (before == 0xFF).all() and (after == 0xFF).all()
            if o.name in ("x", "bias"):
                assert np.isnan(after[:8].view(np.float16)).all()
        else:
            assert (before == A.PATTERN).all() and (after == A.PATTERN).all()
            assert (img[off:off + n] == (0xFF if o.kind == "out" else 0x00)).all()


# ---- the harness on fake entries -----------------------------------------------------------------------------------------------------------
M_, N_, K_ = 5, 7, 64


def fake_case(kind):
    """y[m, n] = sum_k x[m, k] * 2^(scales[n] - 127) in fp16, on numpy memory.  kind: 'good', 'overrun' (stores one element past y),
    'poison' (reads one scale byte past scales), 'zero_ws' (accumulates into a workspace it never cleared)."""
    g = A.gen(1, 2, 3)
    x = (torch.randint(-8, 9, (M_, K_), generator=g) / 8).half()  # sums of eighths: exact in fp32 in any order
    s = torch.randint(120, 130, (N_,), generator=g, dtype=torch.int32).to(torch.uint8)
    ops = [A.In("x", x, 16, K_ * 2), A.In("scales", s, 1, 1), A.Out("y", M_ * N_ * 2, 2, N_ * 2), A.Ws(M_ * 4)]

    def fake(mem, a):
        xv = mem[a("x"):a("x") + M_ * K_ * 2].view(np.float16).reshape(M_, K_).astype(np.float32)
        n_sc = N_ + 1 if kind == "poison" else N_
        sc = mem[a("scales"):a("scales") + n_sc].astype(np.float32)
        ws = mem[a("workspace"):a("workspace") + M_ * 4].view(np.float32)
        if kind != "zero_ws":
            ws[:] = 0
        ws += xv.sum(axis=1)
        scale = np.exp2(sc[:N_] - 127) * (1 + sc[N_] / 255 if kind == "poison" else 1)  # the byte past scales: 0xFF in the arena
        y = (ws[:, None] * scale[None, :]).astype(np.float16)
        n_out = M_ * N_ + (1 if kind == "overrun" else 0)
        mem[a("y"):a("y") + n_out * 2] = np.resize(y.reshape(-1), n_out).view(np.uint8)
        return 0

    def gate(outs):
        want = (x.float().sum(dim=1)[:, None] * torch.exp2(s.float() - 127)[None, :]).half()
        assert torch.equal(A.bt(outs["y"], torch.float16, (M_, N_)), want)

    return A.Case("fake_" + kind, kind, ops, None, gate, fake=fake)


def test_harness_passes_a_correct_entry():
    A.check(fake_case("good"), A.NumpyBackend())


@pytest.mark.parametrize("kind,needle", [("overrun", "0 from the end of y"), ("poison", "y differs from the tight call"), ("zero_ws", "y differs from the tight call")])
def test_harness_reports_a_faulty_entry(kind, needle):
    bad, _ = A.verify(fake_case(kind), A.NumpyBackend())
    assert bad and any(needle in b for b in bad), bad
    with pytest.raises(AssertionError):
        A.check(fake_case(kind), A.NumpyBackend())


def test_harness_reports_a_return_code_and_an_element_never_written():
    c = fake_case("good")
    c.fake = lambda mem, a: -4
    assert any("returned -4" in b for b in A.verify(c, A.NumpyBackend())[0])
    c = fake_case("good")
    c.fake = lambda mem, a: 0  # writes nothing: y keeps its 0xFF fill, identical in the arena and the tight run, NaN at the gate
    with pytest.raises(AssertionError):
        A.check(c, A.NumpyBackend())


def test_refusals_are_counted_and_a_call_that_is_not_refused_is_reported():
    c = fake_case("good")
    c.fake = lambda mem, a: A.INVALID_ARG if (a("x") % 16 or a("y") % 2 or a("workspace") % 16) else 0
    assert A.refusals(c, A.NumpyBackend()) == 3
    c.fake = lambda mem, a: A.INVALID_ARG if a("x") % 16 else 0
    with pytest.raises(AssertionError):
        A.refusals(c, A.NumpyBackend())


# ---- the conditions the limit cases rest on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
def test_routing_at_e_1024_hits_the_first_and_last_expert_and_a_thousand_distinct_ones(form):
    T, S, idx = A.routing_e1024(form)
    flat = idx.reshape(-1)
    assert T * S == flat.numel() == (1200 if form else 1024) and idx.dtype == torch.int32
    live = flat[flat >= 0]
    assert live.max() == 1023 and live.min() == 0 and (flat >= -1).all()
    assert len(set(live.tolist())) >= 1000
    skipped = int((flat < 0).sum())
    assert 0.01 < skipped / flat.numel() < 0.05
    assert A.lib().bie_mxfp4_moe_form(flat.numel(), 1024, 17, 32, 0) in (0, 1)
    assert A.tile_count(idx, 1024) <= A.max_tiles(flat.numel(), 1024)


@pytest.mark.parametrize("E", [3, 1024])
def test_routing_at_p_2_22(E):
    T, S = A.PMAX // A.SMAX, A.SMAX
    idx = A.routing_big(T, S, E, A.gen(E, 1))
    flat = idx.reshape(-1)
    assert flat.numel() == A.PMAX and len(set(flat[flat >= 0].tolist())) == E
    assert 0 < int((flat < 0).sum()) < A.PMAX // 1000
    n = A.tile_count(idx, E)
    assert A.PMAX // 128 <= n <= A.max_tiles(A.PMAX, E)
    words = 4 + 3 * A.max_tiles(A.PMAX, E) + A.PMAX  # head, three tables of max_tiles, the pair list
    assert A.lib().bie_mxfp4_moe_workspace_bytes(A.PMAX, E) == (words * 4 + 15) // 16 * 16
    # the worst routing for the bound: one pair on every expert but one, which takes the rest
    worst = torch.zeros(A.PMAX, dtype=torch.int32)
    worst[:E - 1] = torch.arange(1, E, dtype=torch.int32)
    worst[E - 1] = -1
    assert A.tile_count(worst.reshape(T, S), E) <= A.max_tiles(A.PMAX, E)


@pytest.mark.parametrize("dt", A.DTS)
def test_exact_data_is_a_fixed_point_of_every_quantiser_and_stays_below_2_24_quanta(dt):
    g = A.gen(7)
    x = A.exact_x(9, 160, g, dt)
    assert set(x.float().unique().tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0} and (x[:, ::32] == 1).all()
    for fam in ("mxfp4_a4", "mxfp4_a8", "mxfp6_a8", "mxfp6_a6"):
        assert torch.equal(A.FAMS[fam].xhat(x), x.double()), fam  # the activation quantiser and back
    for fmt, fam in (("fp4", "mxfp4"), ("fp6", "mxfp6")):
        q, s = A.exact_w(fmt, 6, 160, g)
        W = A.FAMS[fam].dequant_w(q, s)
        assert set(W.abs().unique().tolist()) == {0.0, 0.5, 1.0} and (s == 127).all() and (W < 0).any()
    # |x w| <= 1 on a 2^-2 grid: K = 2^20 products and a bias of at most 8 are at most 2^22 + 32 quanta, and fp32 holds 2^24 exactly
    assert 4 * (A.KMAX * 1.0 * 1.0 + 8) == A.EXACT_MAX_QUANTA < 1 << 24
    # the experts' exact construction at P = 2^22: integers |x| <= 2 against e2m1 <= 6 under scales 2^-1 .. 2^1, K = 32
    q, s = A.rand_w("fp4", 8, 32, g, 126, 128)
    W = A.FAMS["mxfp4"].dequant_w(q, s)
    assert float(W.abs().max()) <= 12 and torch.equal(W * 4, (W * 4).round()) and 32 * 2 * 12 * 4 < 1 << 24


def test_limit_cases_have_the_shapes_the_header_states_as_maxima():
    text = open(HEADER).read()
    assert "32 <= K <= 2^20" in text and "1 <= E <= 1024" in text and "1 <= S <= 32" in text and "1 <= P <= 2^22" in text
    assert (A.KMAX, A.EMAX, A.SMAX, A.PMAX) == (1 << 20, 1024, 32, 1 << 22)
    L = A.lib()
    for fam in ("mxfp4_a4", "mxfp4_a8", "mxfp6_a8", "mxfp6_a6"):  # the forms the limit cases force exist at their shapes
        assert getattr(L, f"bie_{fam}_form")(65, 5, A.KMAX, 0) == 1 and getattr(L, f"bie_{fam}_form")(1, 5, A.KMAX, 0) == 0
    M, N = 65600, 32800
    assert M * N > 1 << 31 and M // 4 * N * 2 < 1 << 31 and M * 32768 > 1 << 31 and A.PMAX * 520 > 1 << 31 and A.PMAX // 4 * 520 * 2 < 1 << 31


# ---- the size functions ------------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_at_and_just_past_the_stated_maxima():
    L = A.lib()
    KMAX, EMAX, SMAX, PMAX = 1 << 20, 1024, 32, 1 << 22
    for fam in ("mxfp4_a4", "mxfp4_a8", "mxfp6_a8", "mxfp6_a6"):
        lin, moe = getattr(L, f"bie_{fam}_workspace_bytes"), getattr(L, f"bie_{A.MOE_NAME[fam]}_workspace_bytes")
        for form in (0, 1):
            assert lin(65, 5, KMAX, form) > 0 and lin(65, 5, KMAX + 32, form) == 0 and lin(65, 5, 48, form) == 0 and lin(0, 5, 64, form) == 0
        assert moe(PMAX // SMAX, SMAX, EMAX, 32, 0, 1) > 0 and moe(2, 2, 2, KMAX, 1, 1) > 0 and moe(32, SMAX, EMAX, 32, 1, 0) > 0
        assert moe(PMAX // SMAX + 1, SMAX, EMAX, 32, 0, 1) == 0     # P = 2^22 + 32
        assert moe(3, SMAX + 1, 3, 32, 0, 1) == 0 and moe(3, 2, EMAX + 1, 32, 0, 1) == 0 and moe(2, 2, 2, KMAX + 32, 1, 1) == 0
        assert moe(33, SMAX, 3, 32, 0, 0) == 0                      # the decode form stops at P = 1024
    ws = L.bie_mxfp4_moe_workspace_bytes
    assert ws(PMAX, EMAX) > 0 and ws(PMAX + 1, EMAX) == 0 and ws(PMAX, EMAX + 1) == 0 and ws(0, 3) == 0 and ws(1, 1) > 0


# ---- the form knobs ------------------------------------------------------------------------------------------------------------------------------
_KNOB_CHILD = """
import ctypes, os, sys
L = ctypes.CDLL(sys.argv[1])
knob, mine, others, args = sys.argv[2], sys.argv[3], sys.argv[4].split(","), [int(a) for a in sys.argv[5].split(",")]
def form(name):
    f = getattr(L, name)
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_long] * len(args) + [ctypes.c_int]
    return f(*args, 0)
first = [form(mine)] + [form(o) for o in others]
os.environ[knob] = "0"   # putenv: the C library's getenv sees it
second = form(mine)
del os.environ[knob]
print(*first, second, form(mine))
"""


@pytest.mark.parametrize("knob,mine,others,args", [
    ("BIE_MXFP4_A6_FORM", "bie_mx4a6_form", ("bie_mxfp4_a4_form", "bie_mxfp4_a8_form", "bie_mxfp6_a6_form", "bie_mxfp6_a8_form", "bie_mx8a8_form"), (1, 8, 64)),
    ("BIE_MXFP6_MOE_A6_FORM", "bie_mxfp6_moe_a6_form", ("bie_mxfp4_moe_a4_form", "bie_mx4a6_moe_form", "bie_mxfp4_moe_a8_form", "bie_mxfp6_moe_a8_form"),
     (1, 4, 8, 64)),
    ("BIE_MXFP4_FORM", "bie_mxfp4_form", ("bie_mxfp6_form",), (1, 8, 64)),
    ("BIE_MXFP6_FORM", "bie_mxfp6_form", ("bie_mxfp4_form",), (1, 8, 64)),
    ("BIE_MXFP4_MOE_FORM", "bie_mxfp4_moe_form", ("bie_mxfp6_moe_form",), (1, 4, 8, 64)),
    ("BIE_MXFP6_MOE_FORM", "bie_mxfp6_moe_form", ("bie_mxfp4_moe_form",), (1, 4, 8, 64))])
def test_a_form_knob_reaches_its_own_layer_alone_and_is_read_once(knob, mine, others, args):
    """The layers share one host launch path (csrc/mx_scaled_launch.cuh, and csrc/mx_w16_launch.cuh for the weight-only layers, whose four
    form functions are each checked against their twin of the other format) and each keeps a knob cache of its own: without BIE_TUNING, a FORM
    knob set to 1 turns its own layer's plan at M = 1 (P = 1) from the decode form to the prefill form and no other layer's, and the value
    read at the first call stays when the variable changes or goes away afterwards.  A fresh process: the caches live as long as it does."""
    import subprocess
    from bitorch_engine import _hip
    env = {k: v for k, v in os.environ.items() if k != "BIE_TUNING" and not (k.startswith("BIE_MX") and k.endswith("_FORM"))}
    env[knob] = "1"
    p = subprocess.run([sys.executable, "-c", _KNOB_CHILD, _hip.LIB_PATH, knob, mine, ",".join(others), ",".join(map(str, args))],
                       capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split() == ["1"] + ["0"] * len(others) + ["1", "1"], p.stdout
