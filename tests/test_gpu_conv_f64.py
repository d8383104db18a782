"""Every variant of the f32 sparse-conv kernels (csrc/spconv.hip, csrc/spconv_sorted.hip) on the MI355X, element-wise
against a float64 reference computed on the card with plain torch operators (tests/conv_cases.py).

Each case asserts the plan the library chooses, then runs twice through the C entry points (unscene3d_amd._lib, so the
case decides the variant, not the Python dispatcher): once on integer inputs, where the output must equal the reference
bit for bit whatever the tile shape, split count or reduction order, and once on normal inputs within
2**-20 * sum|a||b| per element.  Outputs and workspaces are interior slices of larger buffers whose guards must keep
their pattern; workspaces have exactly the size the matching *_ws_bytes entry point returns.  The last test prints the
largest fraction of the bound each family used (profiles/conv_f64_ratios.txt is that table of one run: a record)."""
import ctypes as C

import pytest
import torch

import conv_cases as cc
from unscene3d_amd._lib import check, lib

pytestmark = pytest.mark.gpu

RATIOS = {}                                   # family -> [largest err / bound, largest err / (2**-24 mag), cases]


def _stream():
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _p(t):
    return None if t is None else t.data_ptr()


def _ids(cases):
    return [c.name for c in cases]


def _compare(family, c, mode, y, ref, mag):
    if mode == "exact":
        bad = torch.nonzero(y.double() != ref)
        assert bad.shape[0] == 0, (family, c.name, "exact", bad.shape[0], "of", y.numel(), "elements differ; first:",
                                   bad[:8].tolist(), y[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
        return
    frac, ulps = cc.bounded_ratios(y, ref, mag)
    r = RATIOS.setdefault(family, [0.0, 0.0, 0])
    r[0], r[1], r[2] = max(r[0], frac), max(r[1], ulps), r[2] + 1
    assert frac <= 1.0, (family, c.name, "bounded", frac)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------- forward, table form
def _gather_gemm(c, t, out, ws):
    check(lib.usc_spconv_gather_gemm(_p(t["x"]), c.rows_in, c.cin, _p(t["W"]), c.K, c.cout, _p(t["nbr"]), c.n,
                                     _p(t["bias"]), out.ptr(), int(c.acc), int(c.wt), ws.ptr(), ws.nbytes, _stream()),
          "usc_spconv_gather_gemm")


def _run_gather(device, family, c):
    assert cc.decoded_plan(lib, c) == c.plan
    ws_bytes = lib.usc_spconv_gather_gemm_ws_bytes(c.n, c.cin, c.cout, c.K)
    for mode in cc.MODES:
        t = cc.to_device(cc.forward_inputs(c, mode), device)
        ref, mag = cc.ref_forward(t["x"], t["W"], t["nbr"], c.n, t["bias"], t["before"], c.wt, exact=mode == "exact")
        out = cc.GuardedF32(c.n, c.cout, device, init=t["before"])
        ws = cc.GuardedWs(ws_bytes, device)
        _gather_gemm(c, t, out, ws)
        torch.cuda.synchronize()
        _compare(family, c, mode, out.t, ref, mag)
        assert out.guards_intact() and ws.guards_intact(), (c.name, mode, "wrote outside its output or workspace")
        if c.repeat:
            out2, ws2 = cc.GuardedF32(c.n, c.cout, device, init=t["before"]), cc.GuardedWs(ws_bytes, device)
            _gather_gemm(c, t, out2, ws2)
            torch.cuda.synchronize()
            assert _same_bits(out.t, out2.t), (c.name, mode, "a second launch gave other bits")


@pytest.mark.parametrize("c", cc.CASES["row"], ids=_ids(cc.CASES["row"]))
def test_row_order_kernels(device, c):
    _run_gather(device, "row-order", c)


@pytest.mark.parametrize("c", cc.CASES["stem"], ids=_ids(cc.CASES["stem"]))
def test_stem_kernel(device, c):
    _run_gather(device, "stem", c)


@pytest.mark.parametrize("c", cc.CASES["compact"], ids=_ids(cc.CASES["compact"]))
def test_tile_compacted_kernel(device, c):
    _run_gather(device, "compact", c)


# ------------------------------------------------------------------------------------------------- mask-sorted kernel
def _rowsort(c, nbr, device):
    perm = cc.GuardedF32(1, c.n, device)                                  # int32 payloads in the same guarded buffers
    tmask = cc.GuardedF32(1, (c.n + 31) // 32, device)
    ws = cc.GuardedWs(lib.usc_rowsort_ws_bytes(c.K, c.n), device)
    check(lib.usc_rowsort_build(_p(nbr), c.K, c.n, perm.ptr(), tmask.ptr(), ws.ptr(), ws.nbytes, _stream()),
          "usc_rowsort_build")
    torch.cuda.synchronize()
    assert perm.guards_intact() and tmask.guards_intact() and ws.guards_intact(), (c.name, "usc_rowsort_build")
    p = perm.raw.long()
    assert torch.equal(torch.sort(p).values, torch.arange(c.n, device=device)), (c.name, "perm is no permutation")
    present = (nbr >= 0)[:, p]                                             # [K, n] in sorted order
    pad = (-c.n) % 32
    present = torch.cat([present, torch.zeros((c.K, pad), dtype=torch.bool, device=device)], 1)
    bits = present.view(c.K, -1, 32).any(2).long()                        # [K, tiles]
    want = (bits << torch.arange(c.K, device=device)[:, None]).sum(0)
    got = tmask.raw.long() & 0xFFFFFFFF
    assert torch.equal(got, want), (c.name, "tile masks are not the OR of their rows' masks")
    return perm, tmask


def _sorted_gemm(c, t, perm, tmask, out, ws, slices_left=None):
    args = (_p(t["x"]), c.rows_in, c.cin, _p(t["W"]), c.K, c.cout, _p(t["nbr"]), perm.ptr(), tmask.ptr(), c.n,
            _p(t["bias"]), out.ptr(), int(c.acc), int(c.wt), ws.ptr(), ws.nbytes)
    if slices_left is None:
        check(lib.usc_spconv_sorted_gemm(*args, _stream()), "usc_spconv_sorted_gemm")
    else:
        check(lib.usc_spconv_sorted_gemm_ex(*args, C.addressof(slices_left), _stream()), "usc_spconv_sorted_gemm_ex")


@pytest.mark.parametrize("c", cc.CASES["sorted"], ids=_ids(cc.CASES["sorted"]))
def test_mask_sorted_kernel(device, c):
    assert cc.decoded_plan(lib, c) == c.plan
    G = int(c.plan.split("/G")[1])
    ws_bytes = lib.usc_spconv_sorted_ws_bytes(c.n, c.cin, c.cout, c.K)
    for mode in cc.MODES:
        t = cc.to_device(cc.forward_inputs(c, mode), device)
        ref, mag = cc.ref_forward(t["x"], t["W"], t["nbr"], c.n, t["bias"], t["before"], c.wt, exact=mode == "exact")
        perm, tmask = _rowsort(c, t["nbr"], device)
        out = cc.GuardedF32(c.n, c.cout, device, init=t["before"])
        ws = cc.GuardedWs(ws_bytes, device)
        _sorted_gemm(c, t, perm, tmask, out, ws)
        torch.cuda.synchronize()
        _compare("sorted", c, mode, out.t, ref, mag)
        assert out.guards_intact() and ws.guards_intact(), (c.name, mode, "wrote outside its output or workspace")
        if c.repeat:
            out2, ws2 = cc.GuardedF32(c.n, c.cout, device, init=t["before"]), cc.GuardedWs(ws_bytes, device)
            _sorted_gemm(c, t, perm, tmask, out2, ws2)
            torch.cuda.synchronize()
            assert _same_bits(out.t, out2.t), (c.name, mode, "a second launch gave other bits")
        if c.slices:
            # no bias, G > 1: the call reports G slices at the start of the workspace and leaves `out` alone; their
            # sum in slice order is the plain entry point's output, bit for bit
            assert G > 1 and not c.bias and not c.acc
            out3, ws3, left = cc.GuardedF32(c.n, c.cout, device), cc.GuardedWs(ws_bytes, device), C.c_int32(-1)
            _sorted_gemm(c, t, perm, tmask, out3, ws3, left)
            torch.cuda.synchronize()
            assert left.value == G, (c.name, left.value)
            assert bool(out3.pattern_rows().all()) and out3.guards_intact() and ws3.guards_intact()
            sl = ws3.interior().view(torch.float32).view(G, c.n, c.cout)
            total = torch.zeros((c.n, c.cout), dtype=torch.float32, device=device)
            for g in range(G):
                total = total + sl[g]
            assert _same_bits(total, out.t), (c.name, mode, "slices do not sum to the plain output")


# ------------------------------------------------------------------------------------------------- pairs form
@pytest.mark.parametrize("c", cc.CASES["pairs"], ids=_ids(cc.CASES["pairs"]))
def test_pairs_form(device, c):
    assert cc.decoded_plan(lib, c) == c.plan
    cap = c.capacity or sum(c.counts)

    def launch(t, out):
        check(lib.usc_spconv_pairs_gemm(_p(t["x"]), c.cin, _p(t["W"]), c.K, c.cout, _p(t["rows_in"]), _p(t["rows_out"]),
                                        _p(t["koff"]), cap, out.ptr(), _stream()), "usc_spconv_pairs_gemm")
        torch.cuda.synchronize()

    for mode in cc.MODES:
        t = cc.to_device(cc.pairs_inputs(c, mode), device)
        ref, mag, written = cc.ref_pairs(t["x"], t["W"], t["rows_in"], t["rows_out"], t["koff"], c.n, exact=mode == "exact")
        out = cc.GuardedF32(c.n, c.cout, device)
        launch(t, out)
        # rows nobody writes keep the pattern, every other row is written (the pattern is a NaN: never a result)
        assert torch.equal(out.pattern_rows(), ~written), (c.name, mode, "rows written that no pair names, or left out")
        _compare("pairs", c, mode, out.t[written], ref[written], mag[written])
        assert out.guards_intact(), (c.name, mode)
        if c.repeat:
            out2 = cc.GuardedF32(c.n, c.cout, device)
            launch(t, out2)
            assert _same_bits(out.t, out2.t)


# ------------------------------------------------------------------------------------------------- weight gradient
def _wgrad(c, t, dW, ws):
    check(lib.usc_spconv_wgrad(_p(t["a"]), c.cin, _p(t["b"]), c.cout, c.K, _p(t["a_idx"]), _p(t["b_idx"]), _p(t["koff"]),
                               cc.wgrad_capacity(c), dW.ptr(), int(c.acc), ws.ptr(), ws.nbytes, _stream()),
          "usc_spconv_wgrad")
    torch.cuda.synchronize()


def _dw_buffer(c, t, device):
    return cc.GuardedF32(c.K * c.cin, c.cout, device, init=None if t["before"] is None else t["before"].view(-1, c.cout),
                         shift=int(c.shift))


@pytest.mark.parametrize("c", cc.CASES["wgrad"], ids=_ids(cc.CASES["wgrad"]))
def test_weight_gradient(device, c):
    assert cc.decoded_plan(lib, c) == c.plan
    rows = cc.wgrad_capacity(c)
    sizes = (lib.usc_spconv_wgrad_ws_bytes_rows(c.K, c.cin, c.cout, rows), lib.usc_spconv_wgrad_ws_bytes(c.K, c.cin, c.cout))
    for mode in cc.MODES:
        t = cc.to_device(cc.wgrad_inputs(c, mode), device)
        ref, mag = cc.ref_wgrad(t["a"], t["b"], c.K, t["a_idx"], t["b_idx"], t["koff"], t["before"], exact=mode == "exact")
        first = None
        for ws_bytes in sizes:                 # the exact need of this capacity (units.hip allocates that), and the bound
            dW, ws = _dw_buffer(c, t, device), cc.GuardedWs(ws_bytes, device)
            assert dW.ptr() % 16 == (4 if c.shift else 0)
            _wgrad(c, t, dW, ws)
            _compare("wgrad", c, mode, dW.t.view(c.K, c.cin, c.cout), ref, mag)
            assert dW.guards_intact() and ws.guards_intact(), (c.name, mode, ws_bytes, "wrote outside dW or its workspace")
            if first is None:
                first = dW
            else:
                assert _same_bits(first.t, dW.t), (c.name, mode, "the result depends on the workspace size")
        if c.repeat:
            dW, ws = _dw_buffer(c, t, device), cc.GuardedWs(sizes[0], device)
            _wgrad(c, t, dW, ws)
            assert _same_bits(first.t, dW.t), (c.name, mode, "a second launch gave other bits")
        if c.background:
            # the background form walks the same work items with at most 8 workgroups along x (process-wide setting)
            dW, ws = _dw_buffer(c, t, device), cc.GuardedWs(sizes[0], device)
            try:
                lib.usc_spconv_wgrad_grid_limit(8)
                _wgrad(c, t, dW, ws)
            finally:
                lib.usc_spconv_wgrad_grid_limit(0)
            assert _same_bits(first.t, dW.t), (c.name, mode, "the background form gave other bits")
            assert dW.guards_intact() and ws.guards_intact(), (c.name, mode, "background form")


@pytest.mark.parametrize("c", cc.CASES["stem_wgrad"], ids=_ids(cc.CASES["stem_wgrad"]))
def test_stem_weight_gradient_table_form(device, c):
    ws_bytes = lib.usc_spconv_wgrad_table_ws_bytes(c.K, c.cin, c.cout)

    def launch(t, dW, ws):
        check(lib.usc_spconv_wgrad_table(_p(t["x"]), c.cin, _p(t["dy"]), c.cout, _p(t["nbr"]), c.K, c.n, dW.ptr(),
                                         int(c.acc), ws.ptr(), ws.nbytes, _stream()), "usc_spconv_wgrad_table")
        torch.cuda.synchronize()

    for mode in cc.MODES:
        t = cc.to_device(cc.stem_wgrad_inputs(c, mode), device)
        ref, mag = cc.ref_wgrad_table(t["x"], t["dy"], t["nbr"], t["before"], exact=mode == "exact")
        dW, ws = _dw_buffer(c, t, device), cc.GuardedWs(ws_bytes, device)
        launch(t, dW, ws)
        _compare("stem wgrad", c, mode, dW.t.view(c.K, c.cin, c.cout), ref, mag)
        assert dW.guards_intact() and ws.guards_intact(), (c.name, mode)
        if c.repeat:
            dW2, ws2 = _dw_buffer(c, t, device), cc.GuardedWs(ws_bytes, device)
            launch(t, dW2, ws2)
            assert _same_bits(dW.t, dW2.t)


@pytest.mark.parametrize("c", cc.CASES["group"], ids=_ids(cc.CASES["group"]))
def test_grouped_weight_gradient_equals_single_launches(device, c):
    """R problems in one grid give the bits of R single launches (accumulate = 1 into the same pre-existing values)."""
    assert cc.decoded_plan(lib, c) == c.plan
    R, rows = c.n, cc.GROUP_ROWS
    a_idx, b_idx, koff = (v.to(device) for v in cc.pairs_from_counts(c.counts, rows, rows, c.seed))
    cap = int(a_idx.shape[0])
    for mode in cc.MODES:
        g = torch.Generator().manual_seed(c.seed + (0 if mode == "exact" else 1))
        probs = []
        for _ in range(R):
            a = (torch.randint(-3, 4, (rows, c.cin), generator=g).float() if mode == "exact"
                 else torch.randn((rows, c.cin), generator=g)).to(device)
            b = (torch.randint(-2, 3, (rows, c.cout), generator=g).float() if mode == "exact"
                 else torch.randn((rows, c.cout), generator=g)).to(device)
            before = (torch.randint(-2, 3, (c.K * c.cin, c.cout), generator=g).float() if mode == "exact"
                      else torch.randn((c.K * c.cin, c.cout), generator=g)).to(device) if c.acc else None
            probs.append((a, b, before))
        grouped = [cc.GuardedF32(c.K * c.cin, c.cout, device, init=p[2]) for p in probs]
        pa = (C.c_void_p * R)(*[p[0].data_ptr() for p in probs])
        pb = (C.c_void_p * R)(*[p[1].data_ptr() for p in probs])
        pw = (C.c_void_p * R)(*[w.ptr() for w in grouped])
        check(lib.usc_spconv_wgrad_group(R, pa, pb, pw, c.cin, c.cout, c.K, _p(a_idx), _p(b_idx), _p(koff), cap,
                                         int(c.acc), _stream()), "usc_spconv_wgrad_group")
        torch.cuda.synchronize()
        ws_bytes = lib.usc_spconv_wgrad_ws_bytes_rows(c.K, c.cin, c.cout, cap)
        for r, (a, b, before) in enumerate(probs):
            ref, mag = cc.ref_wgrad(a, b, c.K, a_idx, b_idx, koff, None if before is None else before.view(c.K, c.cin, c.cout),
                                    exact=mode == "exact")
            _compare("wgrad group", c, mode, grouped[r].t.view(c.K, c.cin, c.cout), ref, mag)
            assert grouped[r].guards_intact(), (c.name, mode, r)
            single, ws = cc.GuardedF32(c.K * c.cin, c.cout, device, init=before), cc.GuardedWs(ws_bytes, device)
            check(lib.usc_spconv_wgrad(_p(a), c.cin, _p(b), c.cout, c.K, _p(a_idx), _p(b_idx), _p(koff), cap, single.ptr(),
                                       int(c.acc), ws.ptr(), ws.nbytes, _stream()), "usc_spconv_wgrad")
            torch.cuda.synchronize()
            assert _same_bits(single.t, grouped[r].t), (c.name, mode, r, "grouped and single launches differ")


# ------------------------------------------------------------------------------------------------- weight transpose
@pytest.mark.parametrize("c", cc.CASES["transpose"], ids=_ids(cc.CASES["transpose"]))
def test_weight_transpose(device, c):
    W = torch.randn((c.K, c.cin, c.cout), generator=torch.Generator().manual_seed(c.seed)).to(device)
    out = cc.GuardedF32(c.K * c.cout, c.cin, device)
    for _ in range(2):                                                          # and a second launch: the same bits
        check(lib.usc_weight_transpose(_p(W), c.K, c.cin, c.cout, c.mirror, out.ptr(), _stream()), "usc_weight_transpose")
        torch.cuda.synchronize()
        assert _same_bits(out.t.view(c.K, c.cout, c.cin), cc.ref_transpose(W, c.mirror)), c.name
        assert out.guards_intact()


def test_print_the_bound_fractions_per_family():
    """A record, not a check: the largest fraction of 2**-20 * mag each family used over its bounded cases, and the
    largest error in units of 2**-24 * mag."""
    print("\nfamily         cases  max |err| / (2^-20 mag)  max |err| / (2^-24 mag)")
    for fam, (frac, ulps, n) in RATIOS.items():
        print(f"{fam:<14} {n:5d}  {frac:23.4f}  {ulps:23.3f}")
