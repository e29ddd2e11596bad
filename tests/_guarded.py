"""Guard bands for single-op tests: a kernel's operands are strided views into an arena whose other bytes belong to someone else.

Two properties of every kernel are checked with this module (tests/test_guard_bands_gpu.py on the device, tests/test_guarded_cpu.py on torch stand-ins):
its result depends only on the logical extent of its operands (rows [0, rows), columns [0, cols) of each ld-strided matrix), and it writes nothing outside
the logical extent of its outputs.  Both are exact: bits are compared through integer views, never with float ==, so NaNs compare like any other pattern.

embed(logical, ld, guard, fill) lays a logical [rows][cols] tensor (16-bit or fp32) into a fresh buffer [guard + rows + guard][ld]; everything that is not
logical (the guard rows in front and behind, columns [cols, ld) of every row) holds `fill`.  A 1-D operand gets `guard` elements on each side.  A fused view
(q|k|v, [K | V], [value | gate]) is embedded as the whole fused matrix: the sibling is data, not padding.

GUARD = 256 rows (elements for vectors) is the tallest tile in the tree, so a bounded over-read lands in the guard, not in another allocation.  It is a
condition of the method, not a knob.

Fills of input surroundings:
    zero   0
    nan    the type's quiet NaN: bf16 0x7FC0, fp16 0x7E00, fp32 0x7FC00000
    huge   the type's largest finite value, sign alternating by element (bf16 0x7F7F, fp16 0x7BFF, fp32 0x7F7FFFFF; odd flat indices negative): a
           neighbour that a max / min instruction swallows when it is NaN, but that still moves a sum
Output buffers are pre-filled, logical region included, with a sentinel NaN of non-canonical payload, so a NaN the kernel produced can be told from a byte
it never touched:
    SENTINEL_16 = 0x7FA5  (a NaN both as bf16 and as fp16)
    SENTINEL_32 = 0x7FC5A5A5
An operand that is updated in place is an input: its surroundings hold the fill, and containment compares them with a snapshot taken before the launch.
Integer index operands, sizes and the weights' logical rows are never poisoned.

Not covered: the MX fp8 entry points (ldx_op_mx_quant, ldx_op_mx_vt_quant, ldx_op_gemm_mx, ldx_op_gemm2_mx, ldx_op_layernorm_mx, ldx_op_attention_mx,
ldx_op_attention_fp8, ldx_op_qk_norm_rope_mx): their byte and E8M0 scale buffers need a poison of their own.
"""
import torch

GUARD = 256
SENTINEL_16 = 0x7FA5
SENTINEL_32 = 0x7FC5A5A5
FILLS = ("zero", "nan", "huge")
_INT = {2: torch.int16, 4: torch.int32}


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _signed(pattern, size):
    return pattern - (1 << 8 * size) if pattern >> (8 * size - 1) else pattern


def fill_values(shape, dtype, fill, device):
    """A tensor of `shape` holding the fill pattern (huge: the sign follows the flat index)."""
    if fill == "zero":
        return torch.zeros(shape, dtype=dtype, device=device)
    if fill == "nan":
        return torch.full(shape, float("nan"), dtype=dtype, device=device)
    if fill == "huge":
        n = 1
        for s in shape:
            n *= s
        sign = 1.0 - 2.0 * (torch.arange(n, device=device) % 2).to(torch.float64)
        return (sign * torch.finfo(dtype).max).to(dtype).reshape(shape)
    raise ValueError(fill)


def sentinel(shape, dtype, device):
    size = torch.empty((), dtype=dtype).element_size()
    pattern = SENTINEL_16 if size == 2 else SENTINEL_32
    return torch.full(shape, _signed(pattern, size), dtype=_INT[size], device=device).view(dtype)


def _place(buf, logical, guard):
    if logical.dim() == 1:
        view = buf[guard:guard + logical.shape[0]]
    else:
        view = buf[guard:guard + logical.shape[0], :logical.shape[1]]
    view.copy_(logical)
    return view


def embed(logical, ld=None, guard=GUARD, fill="zero"):
    """(buffer, view): `logical` ([rows][cols], or 1-D) inside a buffer [guard + rows + guard][ld] (1-D: [guard + n + guard]) whose other elements hold
    `fill`.  view is the strided window of row `guard`, column 0: view.data_ptr() is what the entry point gets."""
    assert logical.dim() in (1, 2) and logical.element_size() in _INT and logical.is_floating_point()
    if logical.dim() == 1:
        assert ld is None
        shape = (guard + logical.shape[0] + guard,)
    else:
        ld = logical.shape[1] if ld is None else ld
        assert ld >= logical.shape[1]
        shape = (guard + logical.shape[0] + guard, ld)
    buf = fill_values(shape, logical.dtype, fill, logical.device)
    return buf, _place(buf, logical, guard)


def embed_output(rows, cols, dtype, device, ld=None, guard=GUARD):
    """(buffer, view) of an output [rows][cols] (cols None: a vector of `rows` elements): every element, logical ones included, is the sentinel."""
    if cols is None:
        buf = sentinel((guard + rows + guard,), dtype, device)
        return buf, buf[guard:guard + rows]
    ld = cols if ld is None else ld
    assert ld >= cols
    buf = sentinel((guard + rows + guard, ld), dtype, device)
    return buf, buf[guard:guard + rows, :cols]


def _outside_mask(buffer, rows, cols, guard):
    mask = torch.ones(buffer.shape, dtype=torch.bool, device=buffer.device)
    if buffer.dim() == 1:
        mask[guard:guard + rows] = False
    else:
        mask[guard:guard + rows, :cols] = False
    return mask


def outside_untouched(buffer, rows, cols, guard=GUARD, before=None):
    """How many elements outside the logical [rows][cols] (cols None: vector) of `buffer` do not hold the sentinel any more — or, for an operand updated in
    place, differ from `before`, the copy of the buffer taken in front of the launch.  Integer comparison."""
    got = _bits(buffer)
    size = buffer.element_size()
    want = _bits(before) if before is not None else _signed(SENTINEL_16 if size == 2 else SENTINEL_32, size)
    return int(((got != want) & _outside_mask(buffer, rows, cols, guard)).sum())


def same_bits(a, b):
    """How many elements of the logical regions a and b differ in their bits (0: identical)."""
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((_bits(a) != _bits(b)).sum())


class Arena:
    """The operands of one launch under one fill.  inp / out / inout register them; four_launches compares what they hold afterwards."""

    def __init__(self, fill, guard=GUARD):
        self.fill, self.guard, self.outs = fill, guard, []

    def inp(self, logical, ld=None):
        return embed(logical, ld, self.guard, self.fill)[1]

    def out(self, rows, cols, dtype, device, ld=None, name="out"):
        buf, view = embed_output(rows, cols, dtype, device, ld, self.guard)
        self.outs.append((name, buf, view, rows, cols, None))
        return view

    def inout(self, logical, ld=None, name="inout"):
        buf, view = embed(logical, ld, self.guard, self.fill)
        rows, cols = (logical.shape[0], None) if logical.dim() == 1 else logical.shape
        self.outs.append((name, buf, view, rows, cols, buf.clone()))
        return view

    def escaped(self):
        return {name: outside_untouched(buf, rows, cols, self.guard, before) for name, buf, _, rows, cols, before in self.outs}

    def views(self):
        return {name: view for name, _, view, _, _, _ in self.outs}


def four_launches(op, sync=None):
    """op(arena) lays out its operands through `arena`, launches once and returns a callable that checks the result against the op's reference (or None).
    It must produce the same logical inputs on every call.  Runs it with (a) zero, (b) zero, (c) nan, (d) huge surroundings and returns
    {"determinism": {output: differing elements of (b) against (a)}, "independence": {(fill, output): ... of (c), (d) against (a)},
     "containment": {(run, output): elements changed outside the logical output}, "sanity": the callable of run (a)}."""
    runs, sanity = [], None
    for i, fill in enumerate(("zero", "zero", "nan", "huge")):
        arena = Arena(fill)
        check = op(arena)
        if sync:
            sync()
        if i == 0:
            sanity = check
        runs.append(arena)
    base = runs[0].views()
    rep = {"determinism": {n: same_bits(v, base[n]) for n, v in runs[1].views().items()},
           "independence": {(r.fill, n): same_bits(v, base[n]) for r in runs[2:] for n, v in r.views().items()},
           "containment": {("abcd"[i] + ":" + r.fill, n): c for i, r in enumerate(runs) for n, c in r.escaped().items()},
           "sanity": sanity}
    return rep


def violations(rep, prop):
    return {k: v for k, v in rep[prop].items() if v}
