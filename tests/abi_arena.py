"""Arena harness for the C entry points of include/bie_hip.h (the ternary and MX sections), shared by test_abi_arena_gpu.py,
test_abi_limits_gpu.py and test_abi_contract_cpu.py.

Every other test reaches the kernels through the Python wrappers, whose pointers come from the caching allocator: 256-byte aligned and
rounded up to 512 bytes.  Here one call's operands are laid out in ONE uint8 buffer, each at an address that has exactly the alignment
the header states and no more, with a guard band on both sides; the entry is called through _hip.lib() with raw addresses.

  layout(ops)         offsets: address mod (2 * align) == align (odd for a 1-byte operand); guards >= 4 KiB and >= 128 rows of the operand
  image(...)          the buffer before the call: PATTERN everywhere, POISON (0xFF: NaN as fp16 / bf16 / E8M0 / E4M3, -6 as FP4, -7.5 as
                      FP6) in the guards of an input, a valid expert number in the guards of idx, 0xFF in every output, the workspace
                      pre-filled with the run's fill byte
  verify(case, be)    runs the arena twice (workspace 0xFF / 0x00) and once on tight copies (512-byte aligned and rounded, what the
                      allocator hands out); returns the list of findings: return code, a changed byte outside the outputs, an output
                      that differs from the tight run's bits or between the two workspace fills
  check(case, be)     asserts verify() is empty, then the operator's existing gate (tests/*_ref.py) on the tight result
  refusals(case, be)  every validated pointer one step below its alignment: BIE_ERR_INVALID_ARG and not a byte changed

  run_tight(case, be) the tight copies alone, for the shapes at the header's maxima whose guards would not fit

The table entries() lists every launching bie_ternary_* / bie_mxfp* entry with its case builder and its grid of cases; EXCLUDED the ones
left out, with the reason (none today).
Backends: TorchBackend (a device buffer, the real library) and NumpyBackend (host memory, for the fake entries of the CPU self-test, whose
"addresses" are offsets into the buffer)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD_MIN = 4096
TILE_ROWS = 128     # the tallest tile of any of these kernels
PATTERN = 0x5A      # guards of outputs, alignment gaps
POISON = 0xFF
TIGHT_ALIGN = 512   # the caching allocator's rounding (and more than its 256-byte alignment)
INVALID_ARG = -1
F16, BF16, F32 = 0, 1, 2
DT_CODE = {torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32}
DTS = [torch.float16, torch.bfloat16]


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def lib():
    from bitorch_engine import _hip
    return _hip.lib()


# ---- operands, cases, layout -------------------------------------------------------------------------------------------------------------
class Op:
    """One pointer argument.  kind 'in' / 'out' / 'ws'; align = the header's stated minimum; row_bytes = the bytes of one row (an element
    for a vector); data = uint8 bytes of an input (or a callable giving them, for inputs another entry has to build on the GPU);
    poison 'ff' or ('idx', e); validated = capi.hip checks the alignment on the host."""

    def __init__(self, name, kind, nbytes, align, row_bytes, data=None, poison="ff", validated=None):
        assert align in (1, 2, 4, 8, 16) and nbytes > 0 and row_bytes > 0
        self.name, self.kind, self.nbytes, self.align, self.row_bytes = name, kind, int(nbytes), align, int(row_bytes)
        self.data, self.poison = data, poison
        self.validated = (align > 1) if validated is None else validated

    @property
    def guard(self):
        return max(GUARD_MIN, TILE_ROWS * self.row_bytes)

    def bytes(self):
        d = self.data() if callable(self.data) else self.data
        d = tb(d) if isinstance(d, torch.Tensor) else np.asarray(d, dtype=np.uint8).reshape(-1)
        assert d.size == self.nbytes, (self.name, d.size, self.nbytes)
        return d


def tb(t):
    """tensor -> its bytes (numpy uint8, flat)."""
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy()


def bt(b, dtype, shape):
    """bytes -> tensor."""
    return torch.from_numpy(np.ascontiguousarray(b).copy()).view(dtype).reshape(shape)


def In(name, t, align, row_bytes, **kw):
    n = t.numel() * t.element_size() if isinstance(t, torch.Tensor) else kw.pop("nbytes")
    return Op(name, "in", n, align, row_bytes, data=t, **kw)


def Out(name, nbytes, align, row_bytes, **kw):
    return Op(name, "out", nbytes, align, row_bytes, **kw)


def Ws(nbytes, align=16):
    return Op("workspace", "ws", nbytes, align, 1)


class Case:
    """entry: the C function; ops: its pointer operands; argv(addr) -> the arguments before `stream` (addr maps an operand's name to its
    address, None for one the case leaves NULL); gate(outs): the operator's existing check on the tight result (outs maps an output's
    name to its bytes), None = compared with the tight call only; ws = (size function, args) of the workspace; fake(mem, addr) replaces
    the library call (CPU self-test)."""

    def __init__(self, entry, tag, ops, argv=None, gate=None, ws=None, fake=None):
        self.entry, self.tag, self.ops, self.argv, self.gate, self.ws, self.fake = entry, tag, ops, argv, gate, ws, fake
        assert len({o.name for o in ops}) == len(ops)

    @property
    def id(self):
        return f"{self.entry}[{self.tag}]"

    def invoke(self, base, mem, lay, shift=None):
        addr = {o.name: base + lay[o.name][0] for o in self.ops}
        for name, by in (shift or {}).items():
            addr[name] += by
        get = lambda n: addr.get(n)  # noqa: E731
        if self.fake is not None:
            return self.fake(mem, get)
        return getattr(lib(), self.entry)(*self.argv(get), None)


def layout(ops, exact=True):
    """-> ({name: (offset, nbytes)}, total).  exact: each offset is congruent to align mod 2 * align, with op.guard bytes of guard on both
    sides that belong to no other operand; not exact: the tight layout, 512-byte aligned and rounded."""
    lay, cur = {}, 0
    for o in ops:
        if exact:
            start = cur + o.guard
            start += (o.align - start) % (2 * o.align)
            cur = start + o.nbytes + o.guard
        else:
            start = cur
            cur = start + -(-o.nbytes // TIGHT_ALIGN) * TIGHT_ALIGN
        lay[o.name] = (start, o.nbytes)
    return lay, -(-cur // TIGHT_ALIGN) * TIGHT_ALIGN


def image(ops, lay, total, ws_fill, exact=True):
    img = np.full(total, PATTERN if exact else 0, dtype=np.uint8)
    for o in ops:
        off, n = lay[o.name]
        if exact and o.kind == "in":
            for lo, hi in ((off - o.guard, off), (off + n, off + n + o.guard)):
                if o.poison == "ff":
                    img[lo:hi] = POISON
                else:  # an int32 that is a valid expert number, in phase with the operand's own words
                    word = np.frombuffer(np.int32(o.poison[1]).tobytes(), dtype=np.uint8)
                    img[lo:hi] = word[(np.arange(lo, hi) - off) % 4]
        if o.kind == "in":
            img[off:off + n] = o.bytes()
        elif o.kind == "out":
            img[off:off + n] = POISON
        else:
            img[off:off + n] = ws_fill
    return img


class NumpyBackend:
    """Host memory; an address is an offset into the buffer."""

    def run(self, img, call):
        mem = img.copy()
        return call(0, mem), mem


class TorchBackend:
    """A device buffer whose base is 512-byte aligned; an address is a device address."""

    def __init__(self, device="cuda"):
        self.device = device

    def run(self, img, call):
        buf = torch.empty(img.size + TIGHT_ALIGN, dtype=torch.uint8, device=self.device)
        shift = (-buf.data_ptr()) % TIGHT_ALIGN
        view = buf[shift:shift + img.size]
        view.copy_(torch.from_numpy(img))
        torch.cuda.synchronize()
        rc = call(view.data_ptr(), None)
        torch.cuda.synchronize()
        return rc, view.cpu().numpy()


def execute(case, be, exact=True, ws_fill=POISON, shift=None):
    lay, total = layout(case.ops, exact)
    img = image(case.ops, lay, total, ws_fill, exact)
    rc, after = be.run(img, lambda base, mem: case.invoke(base, mem, lay, shift))
    return rc, img, after, lay


def _writable(case, lay, total):
    m = np.zeros(total, dtype=bool)
    for o in case.ops:
        if o.kind != "in":
            off, n = lay[o.name]
            m[off:off + n] = True
    return m


def _outs(case, lay, after):
    return {o.name: after[lay[o.name][0]:lay[o.name][0] + o.nbytes].copy() for o in case.ops if o.kind == "out"}


def verify(case, be):
    """-> (findings, outputs of the tight run)."""
    bad = []
    runs = {}
    for what, exact, fill in (("arena, workspace 0xFF", True, 0xFF), ("arena, workspace 0x00", True, 0x00), ("tight", False, 0xFF)):
        rc, img, after, lay = execute(case, be, exact, fill)
        if rc != 0:
            bad.append(f"{case.id} {what}: returned {rc}")
            continue
        changed = (img != after) & ~_writable(case, lay, img.size)
        if changed.any():
            at = int(changed.argmax())
            near = min(case.ops, key=lambda o: min(abs(at - lay[o.name][0]), abs(at - lay[o.name][0] - o.nbytes)))
            bad.append(f"{case.id} {what}: {int(changed.sum())} bytes outside the outputs changed, the first at offset {at} "
                       f"({at - lay[near.name][0]} from the start and {at - lay[near.name][0] - near.nbytes} from the end of {near.name})")
        runs[what] = _outs(case, lay, after)
    tight = runs.get("tight")
    for what, outs in runs.items():
        if what == "tight" or tight is None:
            continue
        for name, b in outs.items():
            if not np.array_equal(b, tight[name]):
                diff = b != tight[name]
                bad.append(f"{case.id} {what}: {name} differs from the tight call in {int(diff.sum())} bytes, the first at byte {int(diff.argmax())}")
    return bad, tight


def check(case, be):
    bad, tight = verify(case, be)
    assert not bad, "\n".join(bad)
    if case.gate is not None:
        case.gate(tight)


def refusals(case, be):
    """Every validated pointer moved to an address that has half its stated alignment."""
    n = 0
    for o in case.ops:
        if not o.validated or o.align < 2:
            continue
        rc, img, after, _ = execute(case, be, True, POISON, shift={o.name: o.align // 2})
        assert rc == INVALID_ARG, f"{case.id}: {o.name} at {o.align // 2} bytes past a {o.align}-byte boundary returned {rc}"
        assert np.array_equal(img, after), f"{case.id}: the refused call ({o.name} misaligned) changed the arena"
        n += 1
    return n


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (1 << 31))


def rand_w(fmt, N, K, g, lo=118, hi=130):
    """tests/test_mxfp4_gpu.py's draw (fp4: [N, K/2]) and tests/sweeps/fuzz_mxfp6.py's (fp6: [N, 3K/4]): every code byte, scale codes lo .. hi."""
    q = torch.randint(0, 256, (N, K // 2 if fmt == "fp4" else K // 32 * 24), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


def es(dt):
    return torch.empty((), dtype=dt).element_size()


class Fam:
    """One MX family: the weight format, the activation format (None = fp16 / bf16), the restatement and the tolerance of its tests."""

    def __init__(self, name, w, act, decode_rows, y_align, refmod, tolmod, quant=None):
        self.name, self.w, self.act, self.decode_rows, self.y_align, self.refmod, self.tolmod, self.quant = name, w, act, decode_rows, y_align, refmod, tolmod, quant

    @property
    def ref(self):
        return _load(self.refmod)

    def w_row(self, K):
        return K // 2 if self.w == "fp4" else K // 32 * 24

    def a_row(self, K):
        return {"fp4": K // 2, "fp8": K, "fp6": K // 32 * 24}[self.act]

    def dequant_w(self, q, s):
        return (_load("mxfp4_ref") if self.w == "fp4" else _load("mxfp6_ref")).dequant(q, s)

    def quantize_act(self, x):
        return self.ref.quantize_act(x)

    def xhat(self, x):
        """What the contraction sees of x, float64."""
        if self.act is None:
            return x.double()
        xq, xs, flag = self.quantize_act(x)
        assert not flag.any()
        return self.ref.dequant_act(xq, xs)

    def tolerance(self, yref, a, n, dt):
        return _load(self.tolmod).tolerance(yref, a, n, dt)


# The weight-only layers' gate is tests/test_mxfp4_gpu.py::check's formula, which mxfp4_a4_ref.tolerance restates ("the weight-only layer's contract").
FAMS = {f.name: f for f in (
    Fam("mxfp4", "fp4", None, 16, 2, None, "mxfp4_a4_ref"),
    Fam("mxfp6", "fp6", None, 32, 2, None, "mxfp4_a4_ref"),
    Fam("mxfp4_a4", "fp4", "fp4", 64, 16, "mxfp4_a4_ref", "mxfp4_a4_ref", "bie_mxfp4_quantize_act"),
    Fam("mxfp4_a8", "fp4", "fp8", 64, 16, "mxfp4_a8_ref", "mxfp4_a8_ref", "bie_mxfp8_quantize_act"),
    Fam("mxfp6_a8", "fp6", "fp8", 64, 16, "mxfp6_ref", "mxfp6_ref", "bie_mxfp8_quantize_act"),
    Fam("mxfp6_a6", "fp6", "fp6", 64, 16, "mxfp6_a6_ref", "mxfp6_a6_ref", "bie_mxfp6_quantize_act"),
)}
ONE_LAUNCH_K = {"mxfp4_a4": 32768, "mxfp4_a8": 16384, "mxfp6_a8": 16384, "mxfp6_a6": 16384}  # the header's bound of each one-launch decode form
MOE_NAME = {"mxfp4": "mxfp4_moe", "mxfp6": "mxfp6_moe", "mxfp4_a4": "mxfp4_moe_a4", "mxfp4_a8": "mxfp4_moe_a8", "mxfp6_a8": "mxfp6_moe_a8",
            "mxfp6_a6": "mxfp6_moe_a6"}


def gate_close(y, yref, a, n, dt, fam, what, dev):
    tol = fam.tolerance(yref, a, n, dt)
    err = (y.to(dev).double() - yref).abs()
    assert torch.isfinite(y).all(), f"{what}: non-finite output (an element never written reads as NaN)"
    assert (err <= tol).all(), f"{what}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


def _dev():
    return "cuda" if torch.cuda.is_available() else "cpu"


def run_tight(case, be):
    """The case on tight copies alone (the shapes at the header's maxima, whose guards would not fit): return code, gate."""
    rc, _, after, lay = execute(case, be, exact=False)
    assert rc == 0, f"{case.id}: returned {rc}"
    outs = _outs(case, lay, after)
    if case.gate is not None:
        case.gate(outs)
    return outs


# Exact data for any K up to 2^20, one construction for every family.  x: values in {0, +-0.5, +-1} with +1 at the head of each block of
# 32, so every block's amax is 1 and x is a fixed point of each activation quantiser (scaled by 2^2 it is {0, 2, 4}: E2M1 and E2M3 values;
# by 2^8 {0, 128, 256}: E4M3 values).  Weights: magnitudes {0, 0.5, 1} under scale code 127 (2^0).  Every product is a multiple of 2^-2
# of magnitude <= 1, so every partial sum of K <= 2^20 products (plus an integer bias, |bias| <= 8) is a multiple of 2^-2 below 2^20 + 8:
# at most 2^22 + 32 quanta, below 2^24, exact in fp32 in any order.  The result is the float64 sum rounded once to the dtype.
EXACT_MAX_QUANTA = (1 << 22) + 32


def exact_x(M, K, g, dt):
    v = (torch.randint(-2, 3, (M, K), generator=g, dtype=torch.int8).to(torch.float16) * 0.5)
    v[:, ::32] = 1.0
    return v.to(dt)


def exact_w(fmt, N, K, g):
    assert K <= 1 << 20
    m = torch.randint(0, 3, (N, K), generator=g, dtype=torch.int32)
    sign = torch.randint(0, 2, (N, K), generator=g, dtype=torch.int32)
    if fmt == "fp4":
        q = _load("mxfp4_ref").pack((m | (sign << 3)).to(torch.uint8))       # E2M1 codes 0, 1, 2 = 0, 0.5, 1
    else:
        q = _load("mxfp6_ref").pack((m * 4 | (sign << 5)).to(torch.uint8))   # E2M3 codes 0, 4, 8 = 0, 0.5, 1
    return q, torch.full((N, K // 32), 127, dtype=torch.uint8)


def gate_exact(y, yref, dt, what):
    assert float(yref.abs().max()) * 4 <= EXACT_MAX_QUANTA
    want = yref.to(dt).cpu()
    assert torch.equal(y, want), f"{what}: {int((y != want).sum())} elements differ from the rounded float64 sum, max {(y.double() - want.double()).abs().max().item()}"


def _xin(fam, x, gemm):
    """The activation operands of a forward (x) or gemm (xq, xs, row_flag) entry."""
    K = x.shape[1]
    if not gemm:
        return [In("x", x, 16, K * x.element_size())]
    xq, xs, flag = fam.quantize_act(x)
    return [In("xq", xq, 16, fam.a_row(K)), In("xs", xs, 1, K // 32), In("row_flag", flag, 1, 1)]


# ---- linear entries ------------------------------------------------------------------------------------------------------------------------
def linear_case(fam, M, N, K, dt, bias, form, gemm=False, gate=True, exact=False, x=None):
    f = FAMS[fam]
    g = gen(M, N, K, DT_CODE[dt], bias, form, gemm, len(fam))
    if exact:
        q, s = exact_w(f.w, N, K, g)
        x = exact_x(M, K, g, dt) if x is None else x.to(dt)
        b = torch.randint(-8, 9, (N,), generator=g).to(dt) if bias else None
    else:
        q, s = rand_w(f.w, N, K, g)
        x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
        b = torch.randn(N, generator=g).to(dt) if bias else None
    ops = _xin(f, x, gemm) + [In("qweight", q, 16, f.w_row(K)), In("scales", s, 1, K // 32), In("e_col", s.amax(dim=1), 1, 1)]
    if bias:
        ops.append(In("bias", b, 2, es(dt)))
    ops.append(Out("y", M * N * es(dt), f.y_align, N * es(dt)))
    entry = f"bie_{fam}_" + ("gemm" if gemm else "linear_forward")
    ws = None
    if f.act is not None and not gemm:
        ws = (f"bie_{fam}_workspace_bytes", (M, N, K, form))
        ops.append(Ws(getattr(lib(), ws[0])(*ws[1])))
    tail = (M, N, K, DT_CODE[dt], form)
    if f.act is None:
        argv = lambda a: (a("x"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y")) + tail  # noqa: E731
    elif gemm:
        argv = lambda a: (a("xq"), a("xs"), a("row_flag"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), None) + tail  # noqa: E731
    else:
        argv = lambda a: (a("x"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), a("workspace")) + tail  # noqa: E731

    def the_gate(outs):
        dev = _dev()
        xh, W = (x.double() if exact else f.xhat(x)).to(dev), f.dequant_w(q, s).to(dev)  # exact: x is a fixed point of the quantiser
        yref, a = xh @ W.t(), xh.abs() @ W.abs().t()
        if bias:
            yref, a = yref + b.to(dev).double(), a + b.to(dev).double().abs()
        if exact:
            gate_exact(bt(outs["y"], dt, (M, N)), yref, dt, entry)
        else:
            gate_close(bt(outs["y"], dt, (M, N)), yref, a, K, dt, f, entry, dev)

    return Case(entry, f"M{M} N{N} K{K} {'bf16' if dt == torch.bfloat16 else 'f16'} bias{int(bias)} form{form}", ops, argv, the_gate if gate else None, ws)


def quantize_act_case(fam, M, K, dt):
    f = FAMS[fam]
    g = gen(M, K, DT_CODE[dt], 77)
    x = (torch.randn((M, K), generator=g) * torch.exp2(torch.randint(-6, 6, (M, 1), generator=g).float())).to(dt)
    if M > 2:
        x[1, :32] = 0.0  # an all-zero block
    ops = [In("x", x, 16, K * es(dt)), Out("xq", M * f.a_row(K), 16, f.a_row(K)), Out("xs", M * (K // 32), 1, K // 32), Out("row_flag", M, 1, 1)]

    def the_gate(outs):
        xq, xs, flag = f.quantize_act(x)
        assert np.array_equal(outs["row_flag"], tb(flag)) and np.array_equal(outs["xs"], tb(xs)) and np.array_equal(outs["xq"], tb(xq)), f.quant

    return Case(f.quant, f"{fam} M{M} K{K} {DT_CODE[dt]}", ops, lambda a: (a("x"), a("xq"), a("xs"), a("row_flag"), M, K, DT_CODE[dt]), the_gate)


def weight_quantize_case(fmt, N, K, dt):
    """bie_mxfp4_quantize / bie_mxfp6_quantize: w in dtype 0 / 1 / 2, 4-byte aligned."""
    ref = _load("mxfp4_ref" if fmt == "fp4" else "mxfp6_ref")
    g = gen(N, K, DT_CODE[dt], 5)
    w = (torch.randn((N, K), generator=g) * torch.exp2(torch.randint(-6, 6, (N, 1), generator=g).float())).to(dt)
    row = K // 2 if fmt == "fp4" else K // 32 * 24
    ops = [In("w", w, 4, K * es(dt)), Out("qweight", N * row, 16, row), Out("scales", N * (K // 32), 1, K // 32)]

    def the_gate(outs):
        codes, scales = ref.quantize(w)
        assert np.array_equal(outs["scales"], tb(scales)) and np.array_equal(outs["qweight"], tb(ref.pack(codes)))

    return Case(f"bie_mx{fmt}_quantize", f"N{N} K{K} dt{DT_CODE[dt]}", ops, lambda a: (a("w"), a("qweight"), a("scales"), N, K, DT_CODE[dt]), the_gate)


def weight_dequant_case(fmt, N, K, dt):
    ref = _load("mxfp4_ref" if fmt == "fp4" else "mxfp6_ref")
    q, s = rand_w(fmt, N, K, gen(N, K, DT_CODE[dt], 6))
    ops = [In("qweight", q, 16, q.shape[1]), In("scales", s, 1, K // 32), Out("w", N * K * es(dt), 4, K * es(dt))]

    def the_gate(outs):
        assert torch.equal(bt(outs["w"], dt, (N, K)), ref.dequant(q, s).to(dt))  # W is exact in fp32: one rounding to dt

    return Case(f"bie_mx{fmt}_dequant", f"N{N} K{K} dt{DT_CODE[dt]}", ops, lambda a: (a("qweight"), a("scales"), a("w"), N, K, DT_CODE[dt]), the_gate)


def col_exp_case(N, K):
    s = torch.randint(0, 256, (N, K // 32), generator=gen(N, K, 8), dtype=torch.int32).to(torch.uint8)
    ops = [In("scales", s, 1, K // 32), Out("e_col", N, 1, 1)]

    def the_gate(outs):
        assert np.array_equal(outs["e_col"], tb(s.amax(dim=1)))  # the largest code; 255 (a NaN block) is the largest there is

    return Case("bie_mxfp4_col_exp", f"N{N} K{K}", ops, lambda a: (a("scales"), a("e_col"), N, K), the_gate)


def blk_exp_case(rows, K, groups):
    s = torch.randint(0, 256, (groups, rows, K // 32), generator=gen(rows, K, groups, 9), dtype=torch.int32).to(torch.uint8)
    ops = [In("scales", s, 1, K // 32), Out("e_blk", groups * (K // 32), 1, K // 32)]

    def the_gate(outs):
        assert np.array_equal(outs["e_blk"], tb(s.amax(dim=1)))

    return Case("bie_mxfp4_blk_exp", f"rows{rows} K{K} groups{groups}", ops, lambda a: (a("scales"), a("e_blk"), rows, K, groups), the_gate)


def grad_case(fmt, M, N, K, dt, exact=False):
    """bie_mxfp4_linear_grad_input / bie_mxfp6_linear_grad_input: gx [M, K] = gy [M, N] . W."""
    f = FAMS["mxfp4" if fmt == "fp4" else "mxfp6"]
    gr = _load("mxfp6_grad_ref")  # its tolerance is the MXFP4 gradient's formula (tests/test_mxfp4_grad_gpu.py::check)
    g = gen(M, N, K, DT_CODE[dt], 11)
    if exact:
        q, s = exact_w(fmt, N, K, g)
        gy = exact_x(M, (N + 31) // 32 * 32, g, dt)[:, :N].contiguous()
    else:
        q, s = rand_w(fmt, N, K, g, 119, 130)
        gy = (torch.randn((M, N), generator=g) * 0.5).to(dt)
    ops = [In("gy", gy, 2, N * es(dt)), In("qweight", q, 16, q.shape[1]), In("scales", s, 1, K // 32), In("e_blk", s.amax(dim=0), 1, 1),
           Out("gx", M * K * es(dt), 16, K * es(dt))]
    entry = f"bie_{f.name}_linear_grad_input"

    def the_gate(outs):
        dev = _dev()
        W, gd = f.dequant_w(q, s).to(dev), gy.to(dev).double()
        ref, a = gd @ W, gd.abs() @ W.abs()
        gx = bt(outs["gx"], dt, (M, K))
        if exact:
            return gate_exact(gx, ref, dt, entry)
        assert torch.isfinite(gx).all()
        assert ((gx.to(dev).double() - ref).abs() <= gr.tolerance(ref, a, N, dt)).all(), entry

    return Case(entry, f"M{M} N{N} K{K} dt{DT_CODE[dt]}", ops,
                lambda a: (a("gy"), a("qweight"), a("scales"), a("e_blk"), a("gx"), M, N, K, DT_CODE[dt]), the_gate)


# ---- expert entries --------------------------------------------------------------------------------------------------------------------------
def routing(T, S, E, g, skip=1):
    """idx [T, S] int32: random experts, `skip` slots set to -1 (the last slot of the first tokens)."""
    idx = torch.randint(0, E, (T, S), generator=g, dtype=torch.int32)
    flat = idx.reshape(-1)
    for i in range(min(skip, flat.numel() - 1 if flat.numel() > 1 else 0)):
        flat[(i * S + S - 1) % flat.numel()] = -1
    return idx


def experts_reference(f, xh, idx, q, s, bias, dev):
    """(y, absprod) float64 [P, N]: mxfp4_moe_ref.experts on the restated operands (the experts' tests reference)."""
    W = torch.stack([f.dequant_w(q[e], s[e]) for e in range(q.shape[0])]).to(dev)
    T, S = idx.shape
    y, a = _load("mxfp4_moe_ref").experts(xh.reshape(T, S, -1) if xh.shape[0] != T else xh, idx, W, bias)
    return y.reshape(T * S, -1), a.reshape(T * S, -1)


def experts_case(fam, T, S, E, N, K, dt, bias, xpp, form, gemm=False, gate=True, idx=None, exact=False):
    f = FAMS[fam]
    P, R = T * S, T * S if xpp else T
    g = gen(T, S, E, N, K, DT_CODE[dt], bias, xpp, form, gemm, len(fam))
    if exact:
        q, s = exact_w(f.w, E * N, K, g)
        x = exact_x(R, K, g, dt)
        b = torch.randint(-8, 9, (E, N), generator=g).to(dt) if bias else None
    else:
        q, s = rand_w(f.w, E * N, K, g)
        x = (torch.randn((R, K), generator=g) * 0.5).to(dt)
        b = torch.randn((E, N), generator=g).to(dt) if bias else None
    q, s = q.reshape(E, N, -1), s.reshape(E, N, -1)
    idx = routing(T, S, E, g) if idx is None else idx
    ops = _xin(f, x, gemm) + [In("idx", idx, 4, 4 * S, poison=("idx", E - 1)), In("qweight", q, 16, f.w_row(K)), In("scales", s, 1, K // 32),
                             In("e_col", s.amax(dim=2), 1, 1)]
    if bias:
        ops.append(In("bias", b, 2, es(dt)))
    ops.append(Out("y", P * N * es(dt), f.y_align, N * es(dt)))
    name = MOE_NAME[fam]
    entry = f"bie_{name}_" + ("gemm" if gemm else "forward")
    L = lib()
    if f.act is None or gemm:  # the routing region alone, and only for the prefill form
        ws = ("bie_mxfp4_moe_workspace_bytes", (P, E)) if form == 1 else None
    else:
        ws = (f"bie_{name}_workspace_bytes", (T, S, E, K, xpp, form))
    if ws:
        ops.append(Ws(getattr(L, ws[0])(*ws[1])))
        # the header: the one-launch decode form (K up to the row that fits the LDS) does not read the workspace, and only a workspace that is read is validated
        ops[-1].validated = not (f.act is not None and not gemm and form == 0 and K <= ONE_LAUNCH_K[fam])
    tail = (T, S, E, N, K, xpp, DT_CODE[dt], form)
    if gemm:
        argv = lambda a: (a("xq"), a("xs"), a("row_flag"), a("idx"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), a("workspace")) + tail  # noqa: E731
    else:
        argv = lambda a: (a("x"), a("idx"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), a("workspace")) + tail  # noqa: E731

    def the_gate(outs):
        dev = _dev()
        yref, a = experts_reference(f, (x.double() if exact else f.xhat(x)).to(dev), idx, q, s, b, dev)
        y = bt(outs["y"], dt, (P, N))
        skipped = idx.reshape(-1) < 0
        assert (y[skipped].view(torch.int16) == 0).all(), f"{entry}: a skipped slot's row is not +0"
        if exact:
            gate_exact(y, yref, dt, entry)
        else:
            gate_close(y, yref, a, K, dt, f, entry, dev)

    tag = f"T{T} S{S} E{E} N{N} K{K} dt{DT_CODE[dt]} bias{int(bias)} xpp{xpp} form{form}"
    return Case(entry, tag, ops, argv, the_gate if gate else None, ws)


def moe_grad_case(fmt, T, S, E, N, K, dt, out_fp32, idx=None):
    f = FAMS["mxfp4" if fmt == "fp4" else "mxfp6"]
    gr = _load("mxfp6_grad_ref")
    P = T * S
    g = gen(T, S, E, N, K, DT_CODE[dt], out_fp32, 13)
    q, s = rand_w(fmt, E * N, K, g, 119, 130)
    q, s = q.reshape(E, N, -1), s.reshape(E, N, -1)
    gy = (torch.randn((P, N), generator=g) * 0.5).to(dt)
    idx = routing(T, S, E, g) if idx is None else idx
    odt = torch.float32 if out_fp32 else dt
    ws = ("bie_mxfp4_moe_workspace_bytes", (P, E))
    ops = [In("gy", gy, 2, N * es(dt)), In("idx", idx, 4, 4 * S, poison=("idx", E - 1)), In("qweight", q, 16, f.w_row(K)),
           In("scales", s, 1, K // 32), In("e_blk", s.amax(dim=1), 1, K // 32), Out("gx", P * K * es(odt), 16, K * es(odt)),
           Ws(getattr(lib(), ws[0])(*ws[1]))]
    entry = f"bie_{f.name}_moe_grad_input"

    def the_gate(outs):
        dev = _dev()
        gx = bt(outs["gx"], odt, (P, K))
        assert torch.isfinite(gx).all()
        flat = idx.reshape(-1)
        for e in range(-1, E):
            rows = (flat == e).nonzero().reshape(-1)
            if e < 0:
                assert (gx[flat < 0] == 0).all(), f"{entry}: a skipped slot's row is not 0"
            elif rows.numel():
                W, gd = f.dequant_w(q[e], s[e]).to(dev), gy[rows].to(dev).double()
                ref, a = gd @ W, gd.abs() @ W.abs()
                assert ((gx[rows].to(dev).double() - ref).abs() <= gr.tolerance(ref, a, N, odt)).all(), (entry, e)

    return Case(entry, f"T{T} S{S} E{E} N{N} K{K} dt{DT_CODE[dt]} fp32{out_fp32}", ops,
                lambda a: (a("gy"), a("idx"), a("qweight"), a("scales"), a("e_blk"), a("gx"), a("workspace"), T, S, E, N, K, DT_CODE[dt], out_fp32),
                the_gate, ws)


# ---- ternary entries --------------------------------------------------------------------------------------------------------------------------
TDTS = [torch.float16, torch.bfloat16, torch.float32]


def rand_trits(N, K, g, p0=0.4):
    t = torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8) * 2 - 1
    return torch.where(torch.rand((N, K), generator=g) < p0, torch.zeros_like(t), t)


def np_pack(t):
    """tests/test_ternary_gpu.py's numpy packer: [2, N, K/8], plane 0 = non-zero, plane 1 = +1, LSB first."""
    t = t.numpy()
    return torch.from_numpy(np.stack([np.packbits(t != 0, axis=1, bitorder="little"), np.packbits(t > 0, axis=1, bitorder="little")]))


def ternary_pack_case(N, K):
    t = rand_trits(N, K, gen(N, K, 21))
    t[0, :8] = torch.tensor([5, -3, 0, 1, -1, 127, -128, 0], dtype=torch.int8)  # any positive value is +1, any negative one -1
    ops = [In("trits", t, 1, K), Out("qweight", 2 * N * K // 8, 4, K // 8, validated=False)]

    def the_gate(outs):
        assert np.array_equal(outs["qweight"], tb(np_pack(torch.sign(t))))

    return Case("bie_ternary_pack", f"N{N} K{K}", ops, lambda a: (a("trits"), a("qweight"), N, K), the_gate)


def ternary_unpack_case(N, K):
    t = rand_trits(N, K, gen(N, K, 22))
    ops = [In("qweight", np_pack(t), 4, K // 8, validated=False), Out("trits", N * K, 1, K)]

    def the_gate(outs):
        assert np.array_equal(outs["trits"], tb(t))

    return Case("bie_ternary_unpack", f"N{N} K{K}", ops, lambda a: (a("qweight"), a("trits"), N, K), the_gate)


def _on_gpu(entry, outs_bytes, *args):
    """Builds an input another entry produces (an image): runs `entry` on allocator memory, returns the bytes of its last pointer argument."""
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") if isinstance(a, np.ndarray) else a for a in args]
    out = torch.empty(outs_bytes, dtype=torch.uint8, device="cuda")
    ptrs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in dev]
    k = max(i for i, a in enumerate(dev) if isinstance(a, torch.Tensor)) + 1
    rc = getattr(lib(), entry)(*ptrs[:k], out.data_ptr(), *ptrs[k:], None)
    torch.cuda.synchronize()
    assert rc == 0, (entry, rc)
    return out.cpu().numpy()


def ternary_image_case(N, K):
    """bie_ternary_fp4_image: compared with the tight call only here; ternary_layer_case gates the image through the layer that reads it."""
    t = rand_trits(N, K, gen(N, K, 23))
    nb = lib().bie_binary_fp4_image_bytes(N, K)
    ops = [In("qweight", np_pack(t), 4, K // 8), Out("image", nb, 16, max(1, nb // N))]
    return Case("bie_ternary_fp4_image", f"N{N} K{K}", ops, lambda a: (a("qweight"), a("image"), N, K), None)


def _ternary_operands(M, N, K, dt, scaled, seed):
    g = gen(M, N, K, DT_CODE[dt], scaled, seed)
    t = rand_trits(N, K, g)
    x = torch.randn((M, K), generator=g).to(dt)
    bias_a = (torch.randn(K, generator=g) * 0.3).to(dt)
    sa = torch.tensor([0.037], dtype=dt) if scaled else None
    alpha = (torch.rand(N, generator=g) * 0.1).to(dt) if scaled else None
    xb = x + bias_a
    D = torch.where(xb >= 0, 1.0, -1.0).double() @ t.double().t()  # tests/test_ternary_gpu.py: signs() and ref_D()
    want = ((D.to(dt) * sa) * alpha) if scaled else D.float()
    return t, x, bias_a, sa, alpha, want


def ternary_fused_case(M, N, K, dt, y_f32):
    t, x, bias_a, sa, alpha, want = _ternary_operands(M, N, K, dt, not y_f32, 24)
    ydt = torch.float32 if y_f32 else dt
    ops = [In("x", x, 16, K * es(dt)), In("bias_a", bias_a, 16, es(dt)), In("qweight", np_pack(t), 4, K // 8)]
    if not y_f32:
        ops += [In("scale_a", sa, es(dt), es(dt), validated=False), In("alpha", alpha, es(dt), es(dt), validated=False)]
    ops.append(Out("y", M * N * es(ydt), es(ydt), N * es(ydt), validated=False))

    def the_gate(outs):
        assert torch.equal(bt(outs["y"], ydt, (M, N)), want)

    return Case("bie_ternary_linear_fused", f"M{M} N{N} K{K} dt{DT_CODE[dt]} f32{y_f32}", ops,
                lambda a: (a("x"), a("bias_a"), a("qweight"), a("scale_a"), a("alpha"), a("y"), M, N, K, DT_CODE[dt], y_f32), the_gate)


def ternary_layer_case(M, N, K, dt, scaled):
    """bie_ternary_linear_layer_fp4 on the images bie_binary_fp4_image_from_values and bie_ternary_fp4_image build (on the GPU, lazily)."""
    t, x, bias_a, sa, alpha, want = _ternary_operands(M, N, K, dt, scaled, 25)
    L = lib()
    nx, nw = L.bie_binary_fp4_image_bytes(M, K), L.bie_binary_fp4_image_bytes(N, K)
    ximage = lambda: _on_gpu("bie_binary_fp4_image_from_values", nx, x.cuda(), bias_a.cuda(), M, K, DT_CODE[dt])  # noqa: E731
    wimage = lambda: _on_gpu("bie_ternary_fp4_image", nw, np_pack(t).cuda(), N, K)  # noqa: E731
    ops = [In("ximage", ximage, 16, max(1, nx // M), nbytes=nx), In("wimage", wimage, 16, max(1, nw // N), nbytes=nw)]
    if scaled:
        ops += [In("scale_a", sa, es(dt), es(dt), validated=False), In("alpha", alpha, es(dt), es(dt), validated=False)]
    ops.append(Out("y", M * N * es(dt), es(dt), N * es(dt), validated=False))

    def the_gate(outs):
        assert torch.equal(bt(outs["y"], dt, (M, N)), want.to(dt))  # unscaled: y = dt(D)

    return Case("bie_ternary_linear_layer_fp4", f"M{M} N{N} K{K} dt{DT_CODE[dt]} scaled{int(scaled)}", ops,
                lambda a: (a("ximage"), a("wimage"), a("scale_a"), a("alpha"), a("y"), M, N, K, DT_CODE[dt]), the_gate)


def ta8_ref_quant(x):
    """tests/test_ternary_a8_gpu.py::ref_quant."""
    xf = x.float()
    a = xf.abs().amax(dim=1).clamp(min=1e-5)
    s = torch.full_like(a, 127.0) / a
    return torch.round(xf * s[:, None]).clamp(-128, 127).to(torch.int8), a / 127.0


def ta8_x(M, K, dt, g):
    return (torch.randn((M, K), generator=g) * torch.rand((M, 1), generator=g) * 4).to(dt)


def ta8_quantize_case(M, K, ldq, dt):
    x = ta8_x(M, K, dt, gen(M, K, ldq, DT_CODE[dt], 31))
    ops = [In("x", x, 16, K * es(dt)), Out("q", M * ldq, 16, ldq), Out("r", M * 4, 4, 4)]

    def the_gate(outs):
        rq, rr = ta8_ref_quant(x)
        q = bt(outs["q"], torch.int8, (M, ldq))
        assert torch.equal(q[:, :K], rq) and (q[:, K:] == 0).all() and torch.equal(bt(outs["r"], torch.float32, (M,)), rr)

    return Case("bie_ternary_a8_quantize", f"M{M} K{K} ldq{ldq} dt{DT_CODE[dt]}", ops, lambda a: (a("x"), a("q"), a("r"), M, K, ldq, DT_CODE[dt]), the_gate)


def ta8_linear_case(M, N, K, dt, raw, gemm, ldq=None, with_alpha=True):
    """bie_ternary_a8_linear_fused (from x) / bie_ternary_a8_linear_gemm (from q, r with row pitch ldq).  raw takes no alpha; without raw
    a NULL alpha is 1."""
    g = gen(M, N, K, DT_CODE[dt], raw, gemm, 32)
    t, x = rand_trits(N, K, g), ta8_x(M, K, dt, g)
    alpha = (torch.rand(N, generator=g) * 0.05 + 0.001).to(dt) if with_alpha and not raw else None
    rq, rr = ta8_ref_quant(x)
    ydt = torch.int32 if raw else dt
    if gemm:
        ldq = ldq or (K + 63) // 64 * 64
        qp = torch.zeros((M, ldq), dtype=torch.int8)
        qp[:, :K] = rq
        ops = [In("q", qp, 16, ldq), In("r", rr, 4, 4)]
    else:
        ops = [In("x", x, 16, K * es(dt))]
    ops.append(In("qweight", np_pack(t), 4, K // 8))
    if alpha is not None:
        ops.append(In("alpha", alpha, 2 if es(dt) == 2 else 4, es(dt), validated=es(dt) == 2))
    ops.append(Out("y", M * N * es(ydt), 16 if gemm else 4, N * es(ydt)))
    tail = (M, N, K, DT_CODE[dt], raw)
    if gemm:
        argv = lambda a: (a("q"), a("r"), ldq, a("qweight"), a("alpha"), a("y")) + tail  # noqa: E731
    else:
        argv = lambda a: (a("x"), a("qweight"), a("alpha"), a("y")) + tail  # noqa: E731

    def the_gate(outs):
        D = (rq.double() @ t.double().t()).long()  # exact: |D| < 2^53
        a = torch.ones(N) if alpha is None else alpha.float()
        want = D.to(torch.int32) if raw else ((D.float() * rr[:, None]) * a[None, :]).to(dt)  # test_ternary_a8_gpu.py::ref_y
        assert torch.equal(bt(outs["y"], ydt, (M, N)), want)

    tag = f"M{M} N{N} K{K} dt{DT_CODE[dt]} raw{raw} ldq{ldq} alpha{int(alpha is not None)}"
    return Case("bie_ternary_a8_linear_" + ("gemm" if gemm else "fused"), tag, ops, argv, the_gate)


def ternary_conv_case(B, C, H, W, OC, k, st, pad, dt, y_f32, mfma):
    """bie_ternary_conv2d_forward_fused / _mfma on the weight images the extension's helpers build (on the GPU, lazily)."""
    g = gen(B, C, H, W, OC, k, st, pad, DT_CODE[dt], y_f32, mfma)
    t = rand_trits(OC, C * k * k, g).reshape(OC, C, k, k)
    x = torch.randn((B, C, H, W), generator=g).to(dt)
    sa = None if y_f32 else torch.tensor([0.037], dtype=dt)
    alpha = None if y_f32 else (torch.rand(OC, generator=g) * 0.1).to(dt)
    OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    ydt = torch.float32 if y_f32 else dt

    def images():
        from bitorch_engine.extensions import ternary_conv2d_cuda as tc
        qw = tc.w_pack(t.cuda())
        if mfma:
            return [tc.weight_fp4_image(qw, C, k)]
        m, p = tc.weight_lanes(qw, C, k)
        return [m, p]

    cache = {}

    def img(i):
        def get():
            if "v" not in cache:
                cache["v"] = [tb(v) for v in images()]
            return cache["v"][i]
        return get

    L = lib()
    ops = [In("x", x, es(dt), W * es(dt), validated=False)]  # the header states no alignment for the conv's x: an element's (both forms load it element by element)
    if mfma:
        nb = L.bie_binary_fp4_image_bytes(OC, C * k * k)
        ops.append(In("wimage", img(0), 16, nb // OC, nbytes=nb))
    else:
        nb = L.bie_binary_conv_weight_lanes_bytes(OC, C, k)
        ops += [In("wlanes_mask", img(0), 16, max(4, nb // OC), nbytes=nb), In("wlanes_pos", img(1), 16, max(4, nb // OC), nbytes=nb)]
    if not y_f32:
        ops += [In("scale_a", sa, es(dt), es(dt), validated=False), In("alpha", alpha, es(dt), es(dt), validated=False)]
    ops.append(Out("y", B * OC * OH * OW * es(ydt), es(ydt), OW * es(ydt), validated=False))
    tail = (B, C, H, W, OC, k, st, pad, 1, DT_CODE[dt], y_f32)
    if mfma:
        argv = lambda a: (a("x"), a("wimage"), a("scale_a"), a("alpha"), a("y")) + tail  # noqa: E731
    else:
        argv = lambda a: (a("x"), a("wlanes_mask"), a("wlanes_pos"), a("scale_a"), a("alpha"), a("y")) + tail  # noqa: E731

    def the_gate(outs):
        s = torch.where(x >= 0, 1.0, -1.0).double()
        sp = torch.nn.functional.pad(s, (pad, pad, pad, pad), value=-1.0)  # padding s = -1
        D = torch.nn.functional.conv2d(sp, t.double(), stride=st)  # tests/test_ternary_conv_gpu.py::ref_D
        want = D.float() if y_f32 else ((D.to(dt) * sa) * alpha.reshape(1, OC, 1, 1))
        assert torch.equal(bt(outs["y"], ydt, (B, OC, OH, OW)), want)

    entry = "bie_ternary_conv2d_forward_" + ("mfma" if mfma else "fused")
    return Case(entry, f"B{B} C{C} H{H} W{W} OC{OC} k{k} st{st} pad{pad} dt{DT_CODE[dt]} f32{y_f32}", ops, argv, the_gate)


# ---- inputs of the limit cases (tests/test_abi_limits_gpu.py; their conditions are checked in tests/test_abi_contract_cpu.py) -------------------
KMAX, EMAX, SMAX, PMAX = 1 << 20, 1024, 32, 1 << 22  # the header's maxima


def routing_e1024(form):
    """-> (T, S, idx) for E = 1024.  form 1: P = 1200 pairs = every expert once, 136 random ones, 40 skipped slots, shuffled.  form 0:
    P = 1024 (the decode form's largest) = every expert once, then 24 of them (never 0 or 1023) replaced by skipped slots."""
    g = gen(1024, form)
    if form:
        flat = torch.cat([torch.randperm(EMAX, generator=g), torch.randint(0, EMAX, (136,), generator=g), torch.full((40,), -1)])
        flat = flat[torch.randperm(1200, generator=g)]
    else:
        flat = torch.randperm(EMAX, generator=g)
        victims = (flat != 0) & (flat != EMAX - 1)
        flat[victims.nonzero().reshape(-1)[::41][:24]] = -1
    return flat.numel() // 2, 2, flat.to(torch.int32).reshape(-1, 2)


def routing_big(T, S, E, g):
    """idx [T, S] for the calls of millions of pairs: random experts, slot 5 of every 97th token skipped."""
    idx = torch.randint(0, E, (T, S), generator=g, dtype=torch.int32)
    idx[::97, 5 % S] = -1
    return idx


def tile_count(idx, E, bm=128):
    """The row tiles the routing makes: ceil(pairs / 128) summed over the experts, plus those of the skipped slots."""
    flat = idx.reshape(-1).long()
    live = flat[(flat >= 0) & (flat < E)]
    counts = torch.bincount(live, minlength=E)
    return int(((counts + bm - 1) // bm).sum()) + (int(flat.numel() - live.numel()) + bm - 1) // bm


def max_tiles(P, E, bm=128):
    """The tile count bie_mxfp4_moe_workspace_bytes sizes the tile table for: every tile holds a pair, and at most one tile per expert (and one of
    the skipped slots) is not full."""
    return min(P, P // bm + E + 1)


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
DECODE_M, PREFILL_M, NS, KS = (1, 17, 33, 64), (65, 129), (1, 17, 20, 130), (32, 160)
BIG = (257, 160, 21846)  # (M, K, N): the 2 x 2 tile instance of the activation-quantised operators, as in their own tests


def linear_grid(fam, gemm=False):
    """(M, N, K, dt, bias, form): the decode form at M = 1 / 17 / 33 / 64 and at the family's largest decode M (the prefill form where M is
    beyond it), the prefill form forced at M = 65 / 129."""
    f = FAMS[fam]
    out = []
    for dt in DTS:
        for bias in (False, True):
            for N in NS:
                for K in KS:
                    out += [(M, N, K, dt, bias, 0 if M <= f.decode_rows else 1) for M in sorted(set(DECODE_M + (f.decode_rows,)))]
                    out += [(M, N, K, dt, bias, 1) for M in PREFILL_M]
    return [(fam,) + c + (gemm,) for c in out]


def experts_grid(fam, gemm=False):
    out = []
    for dt in DTS:
        for T in (1, 5, 70):
            for xpp in (0, 1):
                for form in (0, 1):
                    for bias, (N, K) in ((False, (17, 32)), (True, (130, 160))):
                        out.append((fam, T, 2, 3, N, K, dt, bias, xpp, form, gemm))
    return out


CONV_FORM1 = [(1, 128, 1, 1, 1, 1, 1, 0), (1, 128, 2, 64, 64, 3, 1, 1)]
CONV_FORM2 = [(1, 64, 1, 1, 1, 1, 1, 0), (1, 128, 2, 65, 64, 3, 1, 1)]


def _tern_fused_shapes():
    """The smallest geometry the one-launch predicate takes, a ragged one, and the largest M it takes at that N, K."""
    L = lib()
    m = 1
    while L.bie_ternary_linear_fused_ok(m + 1, 40, 96) and m < 64:
        m += 1
    wide = [(1, 16385, 256)] if L.bie_ternary_linear_fused_ok(1, 16385, 256) else []  # N > 16384: more than one 16-column sweep of the grid
    return [(1, 1, 32), (3, 40, 96), (m, 40, 96)] + wide


def _ta8_fused_shapes():
    L = lib()
    # the row instances 1 / 2 / 4 / 8 at their smallest shapes, and the wide grid (N > 16384) at its narrowest
    shapes = ((1, 1, 32), (2, 33, 96), (3, 33, 96), (4, 33, 160), (8, 40, 96), (1, 16385, 128), (8, 16385, 128))
    return [(M, N, K) for M, N, K in shapes if L.bie_ternary_a8_fused_ok(M, N, K)]


# entry -> (builder, list of argument tuples).  Built lazily: the size functions need the library.
def entries():
    E = {}
    for fam, f in FAMS.items():
        E[f"bie_{fam}_linear_forward"] = (linear_case, linear_grid(fam) + ([(fam, BIG[0], BIG[2], BIG[1], torch.float16, True, 1, False, False)] if f.act else []))
        if f.act:
            E[f"bie_{fam}_gemm"] = (linear_case, linear_grid(fam, True))
        name = MOE_NAME[fam]
        E[f"bie_{name}_forward"] = (experts_case, experts_grid(fam))
        if f.act:
            E[f"bie_{name}_gemm"] = (experts_case, experts_grid(fam, True))
    for fam in ("mxfp4_a4", "mxfp4_a8", "mxfp6_a6"):
        E[FAMS[fam].quant] = (quantize_act_case, [(fam, M, K, dt) for dt in DTS for M in (1, 17, 65, 129) for K in KS])
    for fmt in ("fp4", "fp6"):
        E[f"bie_mx{fmt}_quantize"] = (weight_quantize_case, [(fmt, N, K, dt) for dt in TDTS for N in (1, 17, 130) for K in KS])
        E[f"bie_mx{fmt}_dequant"] = (weight_dequant_case, [(fmt, N, K, dt) for dt in TDTS for N in (1, 17, 130) for K in KS])
        fam = "mxfp4" if fmt == "fp4" else "mxfp6"
        E[f"bie_{fam}_linear_grad_input"] = (grad_case, [(fmt, M, N, K, dt) for dt in DTS for M in (1, 17, 129) for N in (1, 17, 130) for K in KS])
        E[f"bie_{fam}_moe_grad_input"] = (moe_grad_case, [(fmt, T, 2, 3, N, K, dt, o) for dt in DTS for T in (1, 5, 70) for o in (0, 1)
                                                           for N, K in ((17, 32), (130, 160))])
    E["bie_mxfp4_col_exp"] = (col_exp_case, [(N, K) for N in (1, 17, 130, 300) for K in KS])
    E["bie_mxfp4_blk_exp"] = (blk_exp_case, [(rows, K, groups) for rows in (1, 17, 130) for K in KS for groups in (1, 3)])
    E["bie_ternary_pack"] = (ternary_pack_case, [(N, K) for N in (1, 33) for K in (32, 96)])
    E["bie_ternary_unpack"] = (ternary_unpack_case, [(N, K) for N in (1, 33) for K in (32, 96)])
    E["bie_ternary_fp4_image"] = (ternary_image_case, [(N, K) for N in (1, 33, 130) for K in (32, 96)])
    E["bie_ternary_linear_fused"] = (ternary_fused_case, [(M, N, K, dt, f32) for dt in TDTS for f32 in (0, 1) for M, N, K in _tern_fused_shapes()])
    E["bie_ternary_linear_layer_fp4"] = (ternary_layer_case, [(M, N, K, dt, sc) for dt in TDTS for sc in (False, True)
                                                               for M, N, K in ((1, 1, 32), (3, 40, 96), (130, 33, 160))])
    E["bie_ternary_a8_quantize"] = (ta8_quantize_case, [(M, K, ldq, dt) for dt in TDTS for M, K, ldq in ((1, 32, 32), (3, 96, 128), (17, 160, 256), (130, 32, 64))])
    E["bie_ternary_a8_linear_fused"] = (ta8_linear_case, [(M, N, K, dt, raw, False) for dt in TDTS for raw in (0, 1) for M, N, K in _ta8_fused_shapes()]
                                        + [(3, 33, 96, dt, 0, False, None, False) for dt in TDTS])  # a NULL alpha without raw
    E["bie_ternary_a8_linear_gemm"] = (ta8_linear_case, [(M, N, K, dt, raw, True, ldq) for dt in TDTS for raw in (0, 1)
                                                          for M, N, K, ldq in ((1, 1, 32, 64), (3, 33, 96, 192), (130, 40, 160, 192), (129, 257, 64, 64),
                                                                               (1, 48897, 64, 64))]  # 192 column tiles of 256: the 256 x 256 tile instance
                                       + [(3, 33, 96, dt, 0, True, 192, False) for dt in TDTS])
    # (B, C, H, W, OC, k, stride, pad): the smallest geometry bie_ternary_conv2d_form gives each form (one pixel, one output channel, the
    # fewest channels), and the 3 x 3 padded geometries of tests/test_ternary_mx_boundaries_gpu.py on either side of the VALU form's OW bound
    E["bie_ternary_conv2d_forward_fused"] = (ternary_conv_case, [g + (dt, f32, False) for dt in TDTS for f32 in (0, 1) for g in CONV_FORM1])
    E["bie_ternary_conv2d_forward_mfma"] = (ternary_conv_case, [g + (dt, f32, True) for dt in TDTS for f32 in (0, 1) for g in CONV_FORM2])
    return E


# Launching entries of the header's ternary / MX sections that the table leaves out, each with its reason.
EXCLUDED = {}


def cases(entry):
    build, grid = entries()[entry]
    return [build(*a) for a in grid]
