"""The guard-band helper (tests/_guarded.py) must be able to fail: torch stand-ins for kernels that read too far, write too far, or mask a neighbour by
multiplying it with zero are each rejected by the property they violate, and a correct op passes, for 16-bit and fp32 operands.  No GPU needed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guarded as G  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
ROWS, COLS, LD = 5, 12, 16


def _logical(dtype):
    g = torch.Generator().manual_seed(7)
    return torch.randn(ROWS, COLS, generator=g).to(dtype)


def _window(view, r0, r1, c0, c1):
    """Rows [r0, r1) x columns [c0, c1) of the BUFFER behind `view`, relative to the view's origin: how a kernel with a wrong bound sees memory."""
    ld = view.stride(0)
    return torch.as_strided(view, (r1 - r0, c1 - c0), (ld, 1), view.storage_offset() + r0 * ld + c0)


def _op(kind, dtype):
    """Y[r][c] = 2 X[r][c] + rowsum(X[r]) (fp32 arithmetic, stored in `dtype`), with one defect per kind."""
    def op(arena):
        x = arena.inp(_logical(dtype), LD)
        y = arena.out(ROWS, COLS, dtype, "cpu", LD)
        rows, cols = (ROWS + 1, COLS) if kind == "reads_row" else (ROWS, COLS + 1) if kind in ("reads_col", "mul_zero", "max_col") else (ROWS, COLS)
        w = _window(x, 0, rows, 0, cols).float()
        if kind == "mul_zero":                              # the tail column masked with a multiply: 0 * NaN = NaN
            keep = torch.ones(cols); keep[COLS:] = 0
            w = w * keep
        extra = w[ROWS:] * 0.5 if kind == "reads_row" else 0    # a vertical tap on the row behind the last, column by column
        if kind == "max_col":                               # a row maximum over one column too many, on an instruction that drops NaN (fmax): the
            wide = narrow = w[:, 0]                          # NaN neighbour is swallowed, the finite one is not
            for c in range(1, cols):
                wide = torch.fmax(wide, w[:, c])
                narrow = torch.fmax(narrow, w[:, c]) if c < COLS else narrow
            extra = (wide - narrow)[:, None].clamp(max=1.0)
            w = w[:, :COLS]
        res = 2 * w[:ROWS, :COLS] + w[:ROWS].sum(1, keepdim=True) + extra
        y.copy_(res.to(dtype))
        if kind == "writes_past":                           # one element behind the first row
            _window(y, 0, 1, COLS, COLS + 1).fill_(1.0)
        if kind == "writes_row":                            # one row behind the last
            _window(y, ROWS, ROWS + 1, 0, 1).fill_(1.0)

        def sanity():
            xl = _logical(dtype).float()
            assert torch.equal(y, (2 * xl + xl.sum(1, keepdim=True)).to(dtype))
        return sanity
    return op


@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_op_passes_every_property(dtype):
    rep = G.four_launches(_op("ok", dtype))
    for prop in ("determinism", "independence", "containment"):
        assert not G.violations(rep, prop), (prop, rep[prop])
    rep["sanity"]()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["reads_row", "reads_col"])
def test_over_read_is_rejected_by_independence(dtype, kind):
    rep = G.four_launches(_op(kind, dtype))
    bad = G.violations(rep, "independence")
    assert ("nan", "out") in bad and ("huge", "out") in bad        # zero surroundings hide it: (a) still agrees with the reference
    assert not G.violations(rep, "determinism") and not G.violations(rep, "containment")
    rep["sanity"]()


@pytest.mark.parametrize("dtype", DTYPES)
def test_multiply_by_a_masked_zero_is_rejected_under_nan_only(dtype):
    rep = G.four_launches(_op("mul_zero", dtype))
    bad = G.violations(rep, "independence")
    assert ("nan", "out") in bad and ("huge", "out") not in bad   # 0 * NaN is NaN, 0 * finite is 0: the nan fill is the one that sees it
    assert bad[("nan", "out")] == ROWS * COLS                     # the row sum poisons every element
    assert not G.violations(rep, "containment")


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_swallowing_neighbour_is_rejected_under_huge_only(dtype):
    rep = G.four_launches(_op("max_col", dtype))
    bad = G.violations(rep, "independence")
    assert ("huge", "out") in bad and ("nan", "out") not in bad   # why the huge fill exists
    assert not G.violations(rep, "containment")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["writes_past", "writes_row"])
def test_over_write_is_rejected_by_containment(dtype, kind):
    rep = G.four_launches(_op(kind, dtype))
    bad = G.violations(rep, "containment")
    assert len(bad) == 4 and all(v == 1 for v in bad.values())    # one element, in every one of the four runs
    assert not G.violations(rep, "independence") and not G.violations(rep, "determinism")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", G.FILLS)
def test_embed_lays_out_logical_and_fill(dtype, fill):
    x = _logical(dtype)
    buf, view = G.embed(x, LD, fill=fill)
    assert buf.shape == (2 * G.GUARD + ROWS, LD) and view.data_ptr() == buf[G.GUARD].data_ptr() and view.stride() == (LD, 1)
    assert G.same_bits(view, x) == 0
    ref = G.fill_values(buf.shape, dtype, fill, "cpu")
    outside = G._outside_mask(buf, ROWS, COLS, G.GUARD)
    assert int(outside.sum()) == buf.numel() - ROWS * COLS
    assert int(((G._bits(buf) != G._bits(ref)) & outside).sum()) == 0
    o = buf[outside].float()
    if fill == "zero":
        assert bool((o == 0).all())
    elif fill == "nan":
        assert bool(o.isnan().all()) and int((G._bits(buf)[outside] & 0x7FFF if dtype != torch.float32 else G._bits(buf)[outside]).unique().numel()) == 1
    else:
        assert bool(o.isfinite().all()) and bool((o.abs() == torch.finfo(dtype).max).all()) and int((o > 0).sum()) > 0 and int((o < 0).sum()) > 0
    v, vv = G.embed(x[0], fill=fill)
    assert v.shape == (2 * G.GUARD + COLS,) and G.same_bits(vv, x[0]) == 0 and vv.data_ptr() == v[G.GUARD:].data_ptr()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sentinel_is_a_nan_that_is_neither_fill_nor_canonical(dtype):
    buf, view = G.embed_output(ROWS, COLS, dtype, "cpu", LD)
    assert bool(buf.isnan().all()) and G.outside_untouched(buf, ROWS, COLS) == 0
    want = G.SENTINEL_16 if dtype != torch.float32 else G.SENTINEL_32
    assert int(G._bits(buf)[0, 0]) == want
    canonical = G.fill_values((1,), dtype, "nan", "cpu")
    assert int(G._bits(canonical)[0]) != want
    view.fill_(float("nan"))                                    # a NaN the op produced inside its output is not the sentinel ...
    assert G.same_bits(view, G.embed_output(ROWS, COLS, dtype, "cpu", LD)[1]) == ROWS * COLS
    assert G.outside_untouched(buf, ROWS, COLS) == 0            # ... and the surroundings still are
    buf[0, 0] = float("nan")                                    # a canonical NaN written into the guard is seen, although NaN != NaN as floats
    buf[G.GUARD, COLS] = 0.0
    assert G.outside_untouched(buf, ROWS, COLS) == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_operand_is_compared_with_its_snapshot(dtype):
    def op(kind):
        def run(arena):
            h = arena.inout(_logical(dtype), LD, name="h")
            h.copy_((h.float() * 2).to(dtype))
            if kind == "spill":
                _window(h, -1, 0, 3, 4).fill_(3.0)
        return run
    assert not G.violations(G.four_launches(op("ok")), "containment")
    bad = G.violations(G.four_launches(op("spill")), "containment")
    assert len(bad) == 4 and all(v == 1 for v in bad.values())
