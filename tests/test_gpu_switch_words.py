"""GPU: arbitrary switch words against the ORACLE.  The other switch tests compare a member of a mixed engine with a
one-member engine on the same word -- the same kernel code on both sides -- and only the eight words of the log_exp
experiments meet anything outside the engine (test_gpu_logexp.py).  Here 24 words chosen so that every pair of switch
bits meets in all four states (tests/switch_words.py) are held to tests/golden/switch_words_g96.npz, minted from
oracle/greb_oracle.c with its branches keyed on the same bits.  96x48, 1 flux-correction year + 1 scenario year at
680 ppm; nothing here calls the oracle.

The bar, per case and variable: max(TOL, 3 x noise), TOL the project's whole-run tolerance and `noise` the oracle's own
largest monthly RMS against the same source built with contraction (from the fixture, never from the engine).  3 x because
that yardstick perturbs the oracle in one way only, while FAST also re-associates and uses v_rcp and OCML expf/logf.  An
ignored, swapped or mis-ordered bit misses by three orders of magnitude in at least four cases (measured on the oracle).
Every distance is printed, in units of TOL, before anything is asserted; profiles/switch_words_numbers.txt keeps them."""
import numpy as np
import pytest

import switch_words as SW
from conftest import GOLDEN, rms

pytestmark = pytest.mark.gpu

TOL = np.asarray(SW.TOL)


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from greb_climate_model_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def fixture():
    return SW.load_fixture(GOLDEN)


def own_spin_up(eng_mod, inputs, params, words, engine_name, years=1, **kw):
    """Set A's sequencing: the members carry their words from the start.  -> monthly [nm][years][12][5][ny][nx], the rest."""
    e = eng_mod.Engine(inputs, params, members=[{"switches": w} for w in words], **kw)
    try:
        d = e.describe()
        assert d["engine"] == engine_name and d["correction_sets"] == len(words), d
        yf = e.flux_correction(1)
        mon, yr = e.run(years, SW.CO2)
        return mon, yr, yf, np.stack([e.state(m) for m in range(e.nm)])
    finally:
        e.close()


def against_the_fixture(fixture, which, words, mon, label):
    """mon [len(words)][1][12][5][ny][nx].  Prints every distance, then asserts all of them."""
    missed = []
    for m, w in enumerate(words):
        c = fixture[SW.key(which, w)]
        bar = SW.bar(c)
        got = mon[m, 0]
        assert np.isfinite(got).all(), (label, hex(w))
        last = np.asarray([rms(got[-1, i], c["last"][i]) for i in range(5)])
        means = np.abs(got.astype(np.float64).mean(axis=(2, 3)) - c["means"]).max(axis=0)
        print(f"switch-words | {label} | {which} 0x{w:02x} | last-month RMS / TOL " + " ".join(f"{x:7.3f}" for x in last / TOL) +
              " | monthly means / TOL " + " ".join(f"{x:7.3f}" for x in means / TOL) +
              " | bar / TOL " + " ".join(f"{x:5.2f}" for x in bar / TOL))
        for i, v in enumerate(SW.VARS):
            if not last[i] < bar[i]:
                missed.append((hex(w), v, "last-month RMS", last[i], bar[i]))
            if not means[i] < 3 * bar[i]:
                missed.append((hex(w), v, "monthly means", means[i], 3 * bar[i]))
    assert not missed, (label, missed)


# ------------------------------------------------------------------------------------ 1. set A, fused member kernel
@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_set_a_fused(eng_mod, params, inputs, fixture, strict):
    mon = own_spin_up(eng_mod, inputs, params, SW.SET_A, "fused member kernel", strict=strict)[0]
    against_the_fixture(fixture, "a", SW.SET_A, mon, f"fused {'strict' if strict else 'fast'}")


# ------------------------------------------------------------------------------------ 2. set B, shared spin-up
@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_set_b_fused_after_a_shared_spin_up(eng_mod, params, inputs, fixture, strict):
    e = eng_mod.Engine(inputs, params, members=[{} for _ in SW.SET_B], strict=strict)
    try:
        e.flux_correction(1)
        d = e.describe()
        assert d["engine"] == "fused member kernel" and d["correction_sets"] == 1, d
        e.set_member_experiments(list(SW.SET_B))
        assert e.describe()["correction_sets"] == len(SW.SET_B) == 8
        mon, _ = e.run(1, SW.CO2)
    finally:
        e.close()
    against_the_fixture(fixture, "b", SW.SET_B, mon, f"fused {'strict' if strict else 'fast'}")


# ------------------------------------------------------------------------------------ 3. set A, latitude bands
@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_set_a_latitude_bands(eng_mod, params, inputs, fixture, strict):
    """The any-grid engine takes VAPOR_DIFFUSION_ONLY for all of its members or none (test_gpu_members.py keeps that
    refusal): set A as two engines of eight, split by that bit."""
    for bit6 in (0, 0x40):
        words = [w for w in SW.SET_A if (w & 0x40) == bit6]
        assert len(words) == 8
        mon = own_spin_up(eng_mod, inputs, params, words, "latitude bands", strict=strict, multilaunch=True)[0]
        against_the_fixture(fixture, "a", words, mon, f"bands {'strict' if strict else 'fast'}")


# ------------------------------------------------------------------------------------ 4. precedence of the transport bits
@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_transport_precedence_masks_the_lower_bits(eng_mod, params, inputs, strict):
    """NO_CIRCULATION > NO_VAPOR_TRANSPORT > VAPOR_DIFFUSION_ONLY, as in the oracle (test_switch_words_cpu.py): a bit below
    a set one changes nothing, bit for bit."""
    words = (0x10, 0x30, 0x50, 0x70, 0x20, 0x60)
    out = own_spin_up(eng_mod, inputs, params, words, "fused member kernel", strict=strict)
    assert all(np.isfinite(a).all() for a in out)
    for m, first in ((1, 0), (2, 0), (3, 0), (5, 4)):
        for name, a in zip(("monthly", "yearly", "flux yearly", "state"), out):
            assert np.array_equal(a[m], a[first]), (hex(words[m]), hex(words[first]), name)
    assert rms(out[0][4, 0, 11, 1], out[0][0, 0, 11, 1]) > 1e3 * SW.TOL[1]  # (and the two groups are not one: Tair with and without transport)


# ------------------------------------------------------------------------------------ 5. the model's own blow-up
def test_linear_vapour_without_circulation_blows_up_as_in_the_oracle(eng_mod, params, inputs):
    """LW_LINEAR_VAPOR and NO_CIRCULATION with hydrology (0x18) is finite in scenario year 1 and non-finite in years 2 and 3
    -- in the oracle too (test_switch_words_cpu.py): the model's behaviour under that combination, not the port's.  With
    NO_HYDRO added (0x1a) it stays finite.  Where and how many values go is not pinned."""
    mon, yr, yf, state = own_spin_up(eng_mod, inputs, params, (0x18, 0x1a), "fused member kernel", years=3)
    assert np.isfinite(yf).all() and np.isfinite(mon[:, 0]).all() and np.isfinite(yr[:, 0]).all()
    assert np.isfinite(mon[1]).all() and np.isfinite(yr[1]).all() and np.isfinite(state[1]).all()
    assert not np.isfinite(mon[0, 1]).all() and not np.isfinite(mon[0, 2]).all()
