"""GPU: kth_select_rows_{i32,f32} and kth_topk_rows_{i32,f32} in every kernel form and at
the ranks where a row changes branch inside k_rows_reg (csrc/kth_rows.hpp).

The inputs, the model that names their branches and the reasoning are in
tests/rows_edges.py; tests/test_rows_edges_inputs.py proves on the CPU that the matrix
reaches all 36 forms of k_rows_reg and both row loads of k_rows, and that every edge
probe is the boundary it is named for.  Every comparison here is on bits, against one
stable argsort of the documented order keys (rows_edges.Ref), a NaN expected as
0x7FC00000:

  matrix  67 rows (all-equal extremes, signed zeros, infinities, subnormals, NaNs of both
          signs and many payloads, sorted rows, two values, random bit patterns) at 20
          widths from an aligned base and from one an element off: select, top-k
          smallest and largest, with both outputs, values only and columns only;
  wide    the LDS kernel above 4096 columns at five widths, both bases;
  edges   the rows of rows_edges.full_edges / ragged_edges, every row at every probe
          rank of its case.

Outputs sit in poisoned buffers with guard elements on both sides; the guards, the
range of every column index and the input are checked after the calls.  What each
case aims at is tabulated in DESIGN.md "Narrow-row edges".
"""
import numpy as np
import pytest

import rows_edges as E

pytestmark = pytest.mark.gpu

GUARD = 16
POISON_VALS, POISON_IDX = 0x5A5A5A5A, 0xA5A5A5A5


def to_dev(bits, off):
    """The words as an int32 device tensor starting `off` elements past a 16-byte boundary."""
    import torch
    flat = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    base = torch.zeros(flat.size + 2 * GUARD, dtype=torch.int32, device="cuda")
    dev = base[GUARD + off:GUARD + off + flat.size]
    dev.copy_(torch.from_numpy(flat.view(np.int32).copy()))
    assert dev.data_ptr() % 16 == (4 * off) % 16
    return dev


class Out:
    """n poisoned 4-byte elements `off` past a 16-byte boundary, GUARD poisoned elements on either side."""

    def __init__(self, n, off, poison):
        import torch
        self.n, self.off, self.poison = n, off, poison
        self.base = torch.full((n + 2 * GUARD + off,), int(np.uint32(poison).view(np.int32)), dtype=torch.int32,
                               device="cuda")
        self.t = self.base[GUARD + off:GUARD + off + n]
        assert self.t.data_ptr() % 16 == (4 * off) % 16

    def get(self, tag):
        host = self.base.cpu().numpy().view(np.uint32)
        lo = GUARD + self.off
        assert (host[:lo] == self.poison).all() and (host[lo + self.n:] == self.poison).all(), ("guard overwritten", tag)
        return host[lo:lo + self.n]


def ready():
    """Inputs and poisoned outputs are built on torch's stream and the selector runs on its
    own: finish the former before a call is enqueued on the latter."""
    import torch
    torch.cuda.synchronize()


def want_topk(ref, k, largest):
    memo = ref.__dict__.setdefault("_memo", {})
    if (k, largest) not in memo:
        memo[(k, largest)] = ref.topk(k, largest)
    return memo[(k, largest)]


def same_rows(got, want, tag, names=None):
    bad = np.nonzero((got != want).any(axis=1))[0] if got.ndim == 2 else np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, "rows", [names[b] if names else int(b) for b in bad[:6]], "got", [hex(int(x)) for x in got[bad[0]].ravel()[:6]],
                           "want", [hex(int(x)) for x in want[bad[0]].ravel()[:6]])


def check_select(gpu, ref, dev, k, off, tag, names=None):
    rows, cols = ref.bits.shape
    o = Out(rows, off, POISON_VALS)
    ready()
    gpu.rows(dev, rows, cols, k, o.t, f32=ref.dtype == "f32")
    gpu.sync()
    same_rows(o.get(tag), ref.select(k), (tag, "select", k), names)


def check_topk(gpu, ref, dev, k, largest, off, tag, with_vals=True, with_idx=True, names=None):
    rows, cols = ref.bits.shape
    v = Out(rows * k, off, POISON_VALS) if with_vals else None
    i = Out(rows * k, off, POISON_IDX) if with_idx else None
    ready()
    gpu.topk_rows(dev, rows, cols, k, v.t if v else None, i.t if i else None, largest=largest, f32=ref.dtype == "f32")
    gpu.sync()
    want_v, want_i = want_topk(ref, k, largest)
    tag = (tag, "largest" if largest else "smallest", k, "vals" if with_vals else "", "idx" if with_idx else "")
    if with_idx:
        got = i.get(tag).view(np.int32).reshape(rows, k)
        assert got.min() >= 0 and got.max() < cols, (tag, "column out of range", int(got.min()), int(got.max()))
        same_rows(got, want_i, (tag, "idx"), names)
    if with_vals:
        same_rows(v.get(tag).reshape(rows, k), want_v, (tag, "vals"), names)


def unmodified(dev, ref, tag):
    assert np.array_equal(dev.cpu().numpy().view(np.uint32).reshape(ref.bits.shape), ref.bits), ("input modified", tag)


# ------------------------------------------------------------------ the form matrix
@pytest.mark.parametrize("cols", E.WIDTHS)
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_every_form(gpu, dtype, cols):
    """Select and top-k (smallest, largest; both outputs, values only, columns only) of the 67-row
    matrix from an aligned base and from one an element off."""
    ref = E.matrix(dtype, cols)
    for off in E.OFFS:
        dev = to_dev(ref.bits, off)
        tag = (dtype, cols, "off", off)
        for k in E.select_ranks(cols):
            check_select(gpu, ref, dev, k, off, tag)
        for largest in (False, True):
            for k in E.topk_ranks(cols):
                check_topk(gpu, ref, dev, k, largest, off, tag)
                check_topk(gpu, ref, dev, k, largest, off, tag, with_idx=False)
                check_topk(gpu, ref, dev, k, largest, off, tag, with_vals=False)
        unmodified(dev, ref, tag)


@pytest.mark.parametrize("cols", E.WIDE_WIDTHS)
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_wider_selects(gpu, dtype, cols):
    """k_rows (more than 4096 columns): rows on the 16-byte and on the scalar load, decided per row."""
    ref = E.matrix(dtype, cols)
    for off in E.OFFS:
        dev = to_dev(ref.bits, off)
        for k in E.select_ranks(cols):
            check_select(gpu, ref, dev, k, off, (dtype, cols, "off", off))
        unmodified(dev, ref, (dtype, cols, off))


# ------------------------------------------------------------------ the edge rows
@pytest.mark.parametrize("call", E.CALLS)
@pytest.mark.parametrize("cols", E.FULL_WIDTHS + E.RAGGED_WIDTHS)
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_every_edge(gpu, dtype, cols, call):
    """Every edge row of the case at every probe rank of the case; ragged widths from both bases."""
    ref, ranks = E.edge_case(dtype, cols)
    names = [e.name for e in E.edges(dtype, cols)]
    for off in ((0,) if cols in E.FULL_WIDTHS else E.OFFS):
        dev = to_dev(ref.bits, off)
        tag = (dtype, cols, "off", off)
        for k in ranks[call]:
            if call == "select":
                check_select(gpu, ref, dev, k, off, tag, names)
            else:
                check_topk(gpu, ref, dev, k, call == "largest", off, tag, names=names)
        unmodified(dev, ref, tag)
