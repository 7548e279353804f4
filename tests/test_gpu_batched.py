"""Batched stencils at the batch sizes where the benchmark's kernels spend their time.

The HBM-roofline line of bench.py times diffusion_stream_kernel (greb_kernels.hip, 96x48) at batch 16 384 and
dif_rows_kernel (greb_rows.hip, 384 wide) at batch 1 024; the other GPU tests hand them 1 to 37 fields.  Here:

  * 96x48: more fields than the launch has workgroups, so the grid-stride loop of the stream kernel goes round two and
    three times -- the register prefetch of the next field, its `nb < batch` guard, the barrier before LDS is
    overwritten, the chain list and scratch reused from round to round;
  * the call form bench.py times (device pointers, a side stream, several sweeps per call) against the host form;
  * 384x192: batches whose launch order (greb_strip_order.cpp: rows_tasks) holds streaming strips of all three lengths
    the release tuning cuts -- ~20 rows, 9-10 rows, 4-5 rows -- asserted through engine.diffusion_launch_order;
  * every field of a batch with its own winds through advection and circulation (the per-field offset of u / v).

The reference everywhere is the oracle, one field at a time, EVERY field of every batch.  Bars: STRICT bit-exact;
FAST at the bounds the project states for the same operator and grid (cited where they are used).  Measured figures:
profiles/batched_parity_numbers.txt.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32

# workgroups per compute unit of the 96x48 stream kernel in the release library: `wg_per_cu` in launch_diffusion
# (greb_kernels.hip; an environment knob only in -DGREB_TUNING builds, which no test loads)
STREAM_WG_PER_CU = 2

# FAST advection at 96x48 against the oracle.  The project states no bound for it; this one is measured: the largest
# |FAST - oracle| / max |increment| over the 37 fields of test_own_winds_per_field_g96 on an MI355X was 5.537e-05
# (profiles/batched_parity_numbers.txt; every error was within one spacing(max|X|), the quantisation of the sub-cycled
# rows' fl(fl(T + d) - T)).  Rounded up to two digits; the test grants it plus that one spacing(max|X|).
FAST_ADV_REL_G96 = 5.6e-5


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()  # fails loudly if libgreb_hip.so is missing
    return engine


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _clamped(X, W, dr):
    """Points the diffusion result shows at the clamp (src/greb.f90:715): the expression of test_chain_clamp_g384."""
    return int(np.count_nonzero((X > 0) & (dr / np.maximum(W, f32(1e-30)) <= -0.89 * X)))


def _note(line):
    print("batched-parity: " + line)


# ------------------------------------------------------------------------------------ 96x48: the stream kernel
def _stream_grid(eng_mod):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == eng_mod.device_info(0)["cus"]  # the count launch_diffusion sizes its grid with
    return STREAM_WG_PER_CU * cus


def _period(grid, candidates):
    """A period that the grid is no multiple of: fields b, b + grid, b + 2 grid then fall into different classes."""
    return next(p for p in candidates if grid % p)


def _stream_case(inputs, o, grid, batch):
    """`batch` distinct fields.  Workgroup w of the launch sweeps fields w, w + grid, w + 2 grid: the class of the field
    (smooth temperature, smooth vapour, spiky vapour) and the weight (wz_air, wz_vapor, rough random) change from one
    round to the next, spiky after smooth and smooth after spiky."""
    rng = np.random.default_rng(96 + batch)
    wa, wv = o.field(5).copy(), o.field(6).copy()
    ps, pw = _period(grid, (5, 6, 7, 11)), _period(grid, (3, 4, 5, 7))
    X = np.empty((batch, 48, 96), f32)
    W = np.empty((batch, 48, 96), f32)
    spiky = np.zeros(batch, bool)
    for b in range(batch):
        q = (inputs.qclim[31 * b % 730] * (f32(0.9) + f32(0.0001) * f32(b))).astype(f32)
        if b % ps == 0:  # the vapour field of test_stencil_edge_cases_strict: 30 % exact zeros, polar spikes -> clamp
            x = (q * (rng.random((48, 96)) < 0.7)).astype(f32)
            x[0, ::7] = f32(0.05); x[47, 3::5] = f32(0.08); x[5, 90:] = f32(0.03)
            spiky[b] = True
        elif b % 2:
            x = q
        else:
            x = (inputs.tclim[7 * b % 730] + f32(0.03125) * f32(b)).astype(f32)
        X[b] = x
        wsel = b % pw % 3  # (pw is 3 unless the grid is a multiple of it)
        W[b] = wa if wsel == 0 else wv if wsel == 1 else (f32(0.05) + rng.random((48, 96)).astype(f32) * f32(0.95)).astype(f32)
    ref = np.stack([o.diffusion(X[b], W[b]) for b in range(batch)])
    return {"grid": grid, "batch": batch, "X": X, "W": W, "spiky": spiky, "ref": ref, "host": {}}


@pytest.fixture(scope="module")
def stream_cases(eng_mod, params, inputs, oracle_lib):
    grid = _stream_grid(eng_mod)
    o = oracle_lib.Oracle(inputs, params)
    cases = {name: _stream_case(inputs, o, grid, batch) for name, batch in (("grid+1", grid + 1), ("2grid+37", 2 * grid + 37))}
    o.close()
    return cases


def _stream_host(eng_mod, params, case, strict):
    """engine.diffusion on host arrays, once per case and arithmetic mode."""
    if strict not in case["host"]:
        case["host"][strict] = eng_mod.diffusion(case["X"], case["W"], params, strict=strict)
    return case["host"][strict]


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name", ["grid+1", "2grid+37"])
def test_stream_kernel_past_one_round(eng_mod, params, stream_cases, name, strict):
    """diffusion_stream_kernel with more fields than workgroups: grid + 1 fields (one workgroup goes round twice, the
    prefetch guard `nb < batch` at its edge) and 2 grid + 37 (37 workgroups three times, the others twice).  Every field
    against the oracle: STRICT bit-exact, FAST within the bound test_stencil_edge_cases_strict grants FAST diffusion."""
    c = stream_cases[name]
    grid, batch, X, W, ref, spiky = c["grid"], c["batch"], c["X"], c["W"], c["ref"], c["spiky"]
    rounds = (batch - 1) // grid + 1
    assert rounds == (2 if name == "grid+1" else 3) and batch > (rounds - 1) * grid
    last = batch - (rounds - 1) * grid  # workgroups that go round `rounds` times
    assert last == (1 if name == "grid+1" else 37)
    # the inputs alone: every field distinct; what a workgroup sees in consecutive rounds differs in field, weight and
    # REFERENCE RESULT -- a kernel that served a stale or wrong-round field cannot pass
    assert len({X[b].tobytes() for b in range(batch)}) == batch
    for b in range(batch - grid):
        assert not np.array_equal(W[b], W[b + grid]) and not np.array_equal(ref[b], ref[b + grid]), b
    late = np.arange(grid, batch)
    n_clamped = sum(_clamped(X[b], W[b], ref[b]) for b in np.flatnonzero(spiky))
    n_clamped_late = sum(_clamped(X[b], W[b], ref[b]) for b in np.flatnonzero(spiky) if b >= grid)
    assert n_clamped > 0  # the chain rows' clamp path runs ...
    if rounds == 3:  # ... in second and third rounds too, spiky after smooth and smooth after spiky in one workgroup
        assert (spiky[late] & ~spiky[late - grid]).any() and (~spiky[late] & spiky[late - grid]).any()
        assert n_clamped_late > 0 and any(_clamped(X[b], W[b], ref[b]) for b in np.flatnonzero(spiky) if b >= 2 * grid)
    else:            # (one field in the second round: smooth, after a spiky one)
        assert spiky[0] and not spiky[grid]

    got = _stream_host(eng_mod, params, c, strict)
    worst = 0.0
    for b in range(batch):
        if strict:
            assert np.array_equal(got[b], ref[b]), (name, "field", b, "round", b // grid, "workgroup", b % grid)
        else:
            err = np.abs(got[b].astype(np.float64) - ref[b]).max()
            bound = 4e-6 * max(np.abs(ref[b]).max(), 1e-30) + np.spacing(np.abs(X[b]).max())
            worst = max(worst, float(err / bound))
            assert err <= bound, (name, "field", b, "round", b // grid, "workgroup", b % grid, err, bound)
    _note(f"96x48 stream {'STRICT' if strict else 'FAST'} batch {batch} = {name}: grid {grid}, {last} workgroups x {rounds} rounds, "
          f"the others x {rounds - 1}; {int(spiky.sum())} spiky fields, {n_clamped} clamped points ({n_clamped_late} in rounds >= 2); "
          + ("bit-exact" if strict else f"max FAST error {worst:.3f} of its bound"))


@pytest.mark.parametrize("strict", [True, False])
def test_stream_kernel_device_form_on_a_side_stream(eng_mod, params, stream_cases, strict):
    """The call form bench.py times (timed_sweeps): device pointers, nothing allocated between launches, three sweeps in
    one call, a stream that is not the default one.  dX starts as NaN; after the stream is done it is bit for bit what the
    host form returned for the same 2 grid + 37 fields."""
    import torch
    c = stream_cases["2grid+37"]
    want = _stream_host(eng_mod, params, c, strict)
    T1, wz = torch.from_numpy(c["X"]).cuda(), torch.from_numpy(c["W"]).cuda()
    dX = torch.full_like(T1, float("nan"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    eng_mod.diffusion_dev(params, 96, 48, c["batch"], T1.data_ptr(), wz.data_ptr(), dX.data_ptr(), strict, 3, side.cuda_stream)
    side.synchronize()
    got = dX.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(T1.cpu().numpy(), c["X"]) and np.array_equal(wz.cpu().numpy(), c["W"])  # inputs untouched


# ------------------------------------------------------------------------------------ 384 wide: the row strips
def _streaming_rows(grid):
    """The run of single-sweep rows around the equator (rows_tasks: the streaming region), from the oracle's tables."""
    t2, ny = grid["dif_time2"], len(grid["dif_time2"])
    ks = ke = ny // 2
    if t2[ny // 2] != 1:
        return ks, ke
    while ks > 0 and t2[ks - 1] == 1:
        ks -= 1
    while ke < ny and t2[ke] == 1:
        ke += 1
    return ks, ke


def _strips_by_field(order, batch, ks, ke):
    """Per field the lengths of its strips that lie in the streaming region [ks, ke)."""
    field, k0, k1, _ = order
    out = [[] for _ in range(batch)]
    for fld, a, b in zip(field, k0, k1):
        if fld >= 0 and ks <= a and b <= ke:
            out[fld].append(int(b - a))
    return out


def _levels(strips):
    """Which fields stream in long (>= 18 rows), medium (8-11) and short (<= 5) strips only."""
    long_ = [i for i, s in enumerate(strips) if s and min(s) >= 18]
    medium = [i for i, s in enumerate(strips) if s and min(s) >= 8 and max(s) <= 11]
    short = [i for i, s in enumerate(strips) if s and max(s) <= 5]
    return long_, medium, short


def _rows_case(inp, o, batch, special_every=6):
    """`batch` distinct fields at the oracle's grid (384 wide): temperature (wz_air) and vapour (wz_vapor) in turn, every
    `special_every`-th one a vapour field with exact zeros and spikes or a temperature field with holes -- in the polar
    chain rows as in test_chain_clamp_g384 AND inside the streaming region, where the clamp is dif_sweep_fast's (the
    holes, wider than the stencil, send whole rows through its checked update: 0 <= -0 selects -0.9 * 0)."""
    ny, nx = inp.ny, inp.nx
    g = o.grid()
    ks, ke = _streaming_rows(g)
    rng = np.random.default_rng(384 + batch + ny)
    wa, wv = o.field(5).copy(), o.field(6).copy()
    X = np.empty((batch, ny, nx), f32)
    W = np.empty((batch, ny, nx), f32)
    special = np.zeros(batch, bool)
    mid = list(range(ks + 1, ke - 1, max(1, (ke - ks) // 12))) + ([ke - 2] if ke - ks > 3 else [])  # rows inside the streaming region
    for b in range(batch):
        if special_every and b % special_every == 3:
            special[b] = True
            if (b // special_every) % 2 == 0:
                q = (inp.qclim[31 * b % 730] * f32(0.95)).astype(f32)
                x = (q * (rng.random(q.shape) < 0.7)).astype(f32)  # 30 % exact zeros, everywhere
                x[1, ::7] = f32(0.05); x[2, 3::5] = f32(0.08); x[ny - 3, 300:] = f32(0.03); x[ny - 2, ::11] = f32(0.06)
                # lone spikes between zeros in single-sweep rows.  One sweep takes 0.6 ccx2 (w(j-1) + w(j+1)) / 2 of such a
                # spike, with ccx2 < 1.5 where a row sweeps once (src/greb.f90:652-654): under weights <= 1 it never
                # reaches the clamp there, so these rows get twice wz_vapor (a weight is an input like any other)
                w = wv.copy()
                for k in mid:
                    x[k, 8::16] = f32(0.06)
                    for d in (1, 2, 3):
                        x[k, 8 - d::16] = f32(0); x[k, 8 + d::16] = f32(0)
                    w[k] = f32(2) * wv[k]
                X[b], W[b] = x, w
            else:
                x = (inp.tclim[7 * b % 730] + f32(0.25) * f32(b)).astype(f32)
                x[1:4, 100:140] = f32(0); x[ny - 4:ny - 1, ::9] = f32(0)  # zeros in the longest chains
                for k in mid[::2]:  # holes wider than the stencil, and single zeros, in single-sweep rows
                    x[k, 200:260] = f32(0); x[k, 5::23] = f32(0)
                X[b], W[b] = x, wa
        elif b % 2 == 0:
            X[b], W[b] = (inp.tclim[7 * b % 730] + f32(0.25) * f32(b)).astype(f32), wa
        else:
            X[b], W[b] = (inp.qclim[31 * b % 730] * (f32(0.9) + f32(0.0005) * f32(b))).astype(f32), wv
    ref = np.stack([o.diffusion(X[b], W[b]) for b in range(batch)])
    return {"X": X, "W": W, "special": special, "ref": ref, "ks": ks, "ke": ke}


def _check_rows_case(eng_mod, p, c, label):
    """STRICT bit-exact and FAST within 4e-6 max|ref| + 2 spacing(max|X|) (the bound of
    test_row_strip_diffusion_ragged_batches_and_other_tables), every field."""
    X, W, ref = c["X"], c["W"], c["ref"]
    batch = len(X)
    assert len({X[b].tobytes() for b in range(batch)}) == batch
    sp = np.flatnonzero(c["special"])
    n_clamped = sum(_clamped(X[b], W[b], ref[b]) for b in sp)
    n_stream = sum(_clamped(X[b][c["ks"]:c["ke"]], W[b][c["ks"]:c["ke"]], ref[b][c["ks"]:c["ke"]]) for b in sp)
    if len(sp):
        assert n_clamped > 0
        if c["ke"] - c["ks"] > 3:
            assert n_stream > 0  # ... and some of them in single-sweep rows
    ds = eng_mod.diffusion(X, W, p, strict=True)
    for b in range(batch):
        assert np.array_equal(ds[b], ref[b]), (label, "field", b, "rows", np.flatnonzero((ds[b] != ref[b]).any(axis=1)))
    del ds
    df = eng_mod.diffusion(X, W, p)
    worst = 0.0
    for b in range(batch):
        err = np.abs(df[b].astype(np.float64) - ref[b])
        bound = 4e-6 * max(np.abs(ref[b]).max(), 1e-30) + 2 * np.spacing(np.abs(X[b]).max())
        worst = max(worst, float(err.max() / bound))
        assert err.max() <= bound, (label, "field", b, "row", int(err.max(axis=1).argmax()), err.max(), bound)
    _note(f"{label}: batch {batch}, {len(sp)} spiky / holed fields, {n_clamped} clamped points ({n_stream} in the streaming "
          f"region); STRICT bit-exact; max FAST error {worst:.3f} of its bound")


def _order_with_all_levels(eng_mod, p, batch, ks, ke):
    """The launch order of `batch` 384x192 fields must hold streaming strips of all three lengths.  If the tuning
    constants change, this fails and names a batch that has them -- it never falls back to the short strips alone."""
    order = eng_mod.diffusion_launch_order(p, 384, 192, batch)
    strips = _strips_by_field(order, batch, ks, ke)
    long_, medium, short = _levels(strips)
    if not (long_ and medium and len(short) >= 24):
        for other in range(8, 1025):
            lv = _levels(_strips_by_field(eng_mod.diffusion_launch_order(p, 384, 192, other), other, ks, ke))
            if lv[0] and lv[1] and len(lv[2]) >= 24 and other % 8:
                pytest.fail(f"batch {batch} no longer has streaming strips of all three lengths; the smallest ragged batch that has: {other}")
        pytest.fail(f"no batch up to 1 024 has streaming strips of >= 18, 8-11 and <= 5 rows: rows_tasks changed, rewrite this test")
    return strips, long_, medium, short


def test_row_strips_at_every_strip_level(eng_mod, oracle_lib, inputs384):
    """dif_rows_kernel at batch 179: 23 groups of eight fields, the last one ragged (three fields).  With the release
    tuning the first groups stream in strips of ~20 rows (a 22-row walk: seven times round the three LDS slots), the
    middle ones in 9-10 rows, the last four groups in 4-5 rows -- asserted from the launch order before anything runs."""
    from greb_climate_model_amd import abi
    p = abi.default_params()
    batch = 179
    o = oracle_lib.Oracle(inputs384, p)
    ks, ke = _streaming_rows(o.grid())
    assert ke - ks >= 120  # most of the field streams
    strips, long_, medium, short = _order_with_all_levels(eng_mod, p, batch, ks, ke)
    # who owns what: whole groups of eight, the long strips in front, the short ones last, nothing else between
    assert long_ == list(range(len(long_))) and len(long_) >= 8 and len(long_) % 8 == 0
    assert medium == list(range(len(long_), len(long_) + len(medium))) and len(medium) % 8 == 0
    assert short == list(range(batch - len(short), batch)) and len(short) >= 24
    assert len(long_) + len(medium) + len(short) == batch
    assert max(max(strips[i]) for i in long_) + 2 >= 20  # the walk of such a strip: its rows and two halo rows
    _note(f"384x192 batch {batch}: streaming rows {ks}-{ke - 1}; fields 0-{long_[-1]} in strips of {sorted(set(sum((strips[i] for i in long_), [])))} rows, "
          f"{medium[0]}-{medium[-1]} in {sorted(set(sum((strips[i] for i in medium), [])))}, {short[0]}-{short[-1]} in {sorted(set(sum((strips[i] for i in short), [])))}")
    c = _rows_case(inputs384, o, batch)
    o.close()
    for level in (long_, medium, short):  # a spiky or holed field at every level
        assert c["special"][level].any()
    _check_rows_case(eng_mod, p, c, "384x192 kappa 8e5")


def test_row_strips_long_strips_beside_1800_sweep_rows(eng_mod, oracle_lib, inputs384):
    """kappa = 6.5e5, batch 168 (21 full groups, the first one at the long strips): 1 800 dependent sweeps in each polar
    row and 180 in the next, so other cap strips run beside the long streaming ones.  Same two bars."""
    from greb_climate_model_amd import abi
    p = abi.default_params()
    p.kappa = 6.5e5
    batch = 168
    o = oracle_lib.Oracle(inputs384, p)
    g = o.grid()
    assert g["dif_time2"][0] == 1800 and g["dif_time2"][1] == 180
    ks, ke = _streaming_rows(g)
    strips, long_, medium, short = _order_with_all_levels(eng_mod, p, batch, ks, ke)
    assert long_ == list(range(8)) and short == list(range(batch - len(short), batch))
    _note(f"384x192 kappa 6.5e5 batch {batch}: streaming rows {ks}-{ke - 1}; fields 0-7 in strips of {sorted(set(sum((strips[i] for i in long_), [])))} rows, "
          f"{len(medium)} fields in {sorted(set(sum((strips[i] for i in medium), [])))}, {len(short)} in {sorted(set(sum((strips[i] for i in short), [])))}")
    c = _rows_case(inputs384, o, batch, special_every=12)  # (every spiky field sends the clamp through 2 x 1 800 oracle sweeps)
    o.close()
    assert c["special"][long_].any() and c["special"][short].any()
    _check_rows_case(eng_mod, p, c, "384x192 kappa 6.5e5")


@pytest.mark.parametrize("ny", [96, 48])
def test_row_strips_on_flatter_384_wide_grids(eng_mod, oracle_lib, ny):
    """rows_supported takes any ny <= 192 at nx = 384; the batched sweep has never been given another one.  19 fields
    at 384x96 and 384x48 against the oracle at that grid: the streaming region is shorter, the caps other rows."""
    from greb_climate_model_amd import abi, workload
    inp = workload.make_inputs(384, ny)
    p = abi.default_params()
    batch = 19
    o = oracle_lib.Oracle(inp, p)
    g = o.grid()
    assert g["subcycled"].all()  # hence the row strips, not the band kernel
    ks, ke = _streaming_rows(g)
    field, k0, k1, up = eng_mod.diffusion_launch_order(p, 384, ny, batch)
    assert len(field) > 0 and field.max() == batch - 1
    cover = np.zeros((batch, ny), np.int32)
    for fld, a, b in zip(field, k0, k1):
        if fld >= 0:
            assert 0 <= a < b <= ny
            cover[fld, a:b] += 1
    assert (cover == 1).all()
    mine = sorted((int(a), int(b)) for fld, a, b in zip(field, k0, k1) if fld == batch - 1)
    caps = [x for x in mine if not (ks <= x[0] and x[1] <= ke)]
    inner = sorted({b - a for a, b in mine if ks <= a and b <= ke})
    _note(f"384x{ny} batch {batch}: sweeps per row from the pole {g['dif_time2'][:ks + 1].tolist()}, streaming rows {ks}-{ke - 1}; "
          f"{len(field)} tasks; the last field: cap strips {caps}, {len(mine) - len(caps)} streaming strips of {inner} rows")
    c = _rows_case(inp, o, batch)
    o.close()
    _check_rows_case(eng_mod, p, c, f"384x{ny}")


# ------------------------------------------------------------------------------------ own winds per field
def _ulp_bars(got, ref, X, n_ulp, label):
    """The FAST bars of test_strict_stencils_bit_exact_g384_vs_reference: every row is sub-cycled, an increment is
    fl(fl(T + d) - T), quantised to ulp(T): n_ulp of the field's largest value at most, half an ulp in the rms."""
    worst = 0.0
    for i in range(len(ref)):
        ulp = float(np.spacing(f32(np.abs(X[i]).max())))
        err = np.abs(got[i].astype(np.float64) - ref[i])
        worst = max(worst, float(err.max() / (n_ulp * ulp)))
        assert err.max() <= n_ulp * ulp and np.sqrt((err ** 2).mean()) < 0.5 * ulp, (label, i, err.max(), ulp)
    return worst


def test_own_winds_per_field_g96(eng_mod, params, inputs, oracle_lib):
    """37 fields at 96x48, each with the winds of another step of the year, every fifth all-westward (u < 0 in the
    sub-cycled rows: the :881 index bug): advection through the band kernel, circulation through
    circulation_g96_kernel, whose u / v are offset per field.  STRICT bit-exact for every field; FAST diffusion and
    circulation at the bounds of test_stencil_edge_cases_strict, FAST advection at FAST_ADV_REL_G96."""
    o = oracle_lib.Oracle(inputs, params)
    wa, wv = o.field(5).copy(), o.field(6).copy()
    n = 37
    X = np.stack([(inputs.tclim[7 * i % 730] + f32(i)).astype(f32) if i % 2 == 0 else
                  (inputs.qclim[31 * i % 730] * (f32(0.9) + f32(0.005) * f32(i))).astype(f32) for i in range(n)])
    W = np.stack([wa if i % 2 == 0 else wv for i in range(n)])
    U = np.stack([inputs.uclim[19 * i % 730] if i % 5 != 4 else (-np.abs(inputs.uclim[19 * i % 730]) - f32(3)).astype(f32) for i in range(n)])
    V = np.stack([inputs.vclim[(19 * i + 365) % 730] if i % 3 else (-inputs.vclim[19 * i % 730]).astype(f32) for i in range(n)])
    assert len({U[i].tobytes() for i in range(n)}) == n and len({V[i].tobytes() for i in range(n)}) == n
    dr = [o.diffusion(X[i], W[i]) for i in range(n)]
    ar = [o.advection(X[i], W[i], u=U[i], v=V[i]) for i in range(n)]
    cr = [o.circulation(X[i], W[i], u=U[i], v=V[i]) for i in range(n)]
    # (the winds matter: with the neighbour's winds the reference result is another)
    assert not any(np.array_equal(ar[i], o.advection(X[i], W[i], u=U[i - 1], v=V[i - 1])) for i in range(1, n))
    o.close()
    a = eng_mod.advection(X, W, U, V, params, strict=True)
    c = eng_mod.circulation(X, W, U, V, params, strict=True)
    for i in range(n):
        assert np.array_equal(a[i], ar[i]), ("advection", i)
        assert np.array_equal(c[i], cr[i]), ("circulation", i)
    df, af, cf = eng_mod.diffusion(X, W, params), eng_mod.advection(X, W, U, V, params), eng_mod.circulation(X, W, U, V, params)
    worst = {"dif": 0.0, "adv": 0.0, "crc": 0.0}
    adv_rel = 0.0
    fails = []
    for i in range(n):
        sp = np.spacing(np.abs(X[i]).max())
        for name, got, ref, bound in (("dif", df[i], dr[i], 4e-6 * max(np.abs(dr[i]).max(), 1e-30) + sp),
                                      ("adv", af[i], ar[i], FAST_ADV_REL_G96 * max(np.abs(ar[i]).max(), 1e-30) + sp),
                                      ("crc", cf[i], cr[i], 1e-5 * max(np.abs(cr[i]).max(), 1e-30) + 24 * sp)):
            err = np.abs(got.astype(np.float64) - ref).max()
            worst[name] = max(worst[name], float(err / bound))
            if name == "adv":
                adv_rel = max(adv_rel, float(err / max(np.abs(ref).max(), 1e-30)))
            if err > bound:
                fails.append((name, i, err, bound))
    _note(f"96x48 own winds, {n} fields: STRICT advection and circulation bit-exact; max FAST error as a fraction of its bound: "
          f"diffusion {worst['dif']:.3f}, advection {worst['adv']:.3f}, circulation {worst['crc']:.3f}; "
          f"FAST advection max |error| / max |increment| = {adv_rel:.3e}")
    assert not fails, fails


def test_own_winds_per_field_g384(eng_mod, oracle_lib, inputs384):
    """Nine fields at 384x192 with their own winds through the band sweep_kernel (advection, circulation) and the row
    strips (diffusion): STRICT bit-exact for all three operators; FAST diffusion and circulation at the ulp bars of
    test_strict_stencils_bit_exact_g384_vs_reference, per field."""
    from greb_climate_model_amd import abi
    inp = inputs384
    p = abi.default_params()
    o = oracle_lib.Oracle(inp, p)
    wa, wv = o.field(5).copy(), o.field(6).copy()
    n = 9
    X = np.stack([(inp.tclim[79 * i % 730] + f32(0.5) * f32(i)).astype(f32) if i % 2 == 0 else
                  (inp.qclim[83 * i % 730] * (f32(0.9) + f32(0.01) * f32(i))).astype(f32) for i in range(n)])
    W = np.stack([wa if i % 2 == 0 else wv for i in range(n)])
    U = np.stack([inp.uclim[(81 * i + 40) % 730] for i in range(n)])
    V = np.stack([inp.vclim[(81 * i + 400) % 730] for i in range(n)])
    assert len({U[i].tobytes() for i in range(n)}) == n and len({V[i].tobytes() for i in range(n)}) == n
    dr = [o.diffusion(X[i], W[i]) for i in range(n)]
    ar = [o.advection(X[i], W[i], u=U[i], v=V[i]) for i in range(n)]
    cr = [o.circulation(X[i], W[i], u=U[i], v=V[i]) for i in range(n)]
    assert not any(np.array_equal(ar[i], o.advection(X[i], W[i], u=U[i - 1], v=V[i - 1])) for i in range(1, n))
    o.close()
    d = eng_mod.diffusion(X, W, p, strict=True)
    a = eng_mod.advection(X, W, U, V, p, strict=True)
    c = eng_mod.circulation(X, W, U, V, p, strict=True)
    for i in range(n):
        assert np.array_equal(d[i], dr[i]), ("diffusion", i)
        assert np.array_equal(a[i], ar[i]), ("advection", i)
        assert np.array_equal(c[i], cr[i]), ("circulation", i)
    wd = _ulp_bars(eng_mod.diffusion(X, W, p), dr, X, 2, "dif")
    wc = _ulp_bars(eng_mod.circulation(X, W, U, V, p), cr, X, 8, "crc")
    _note(f"384x192 own winds, {n} fields: STRICT diffusion, advection and circulation bit-exact; max FAST error as a fraction "
          f"of its bound: diffusion {wd:.3f} of 2 ulp, circulation {wc:.3f} of 8 ulp")
