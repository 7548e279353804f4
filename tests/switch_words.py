"""The switch words that are held to the oracle beyond the ten log_exp experiments, and what the tests of them share
(tests/test_switch_words_cpu.py, tests/test_gpu_switch_words.py, tests/golden/make_golden_switch_words.py).

Every case is 96x48, the synthetic workload, abi.default_params(ipx=95, ipy=38), 1 flux-correction year + 1 scenario
year at 680 ppm.

SET A, own spin-up: the word is set BEFORE the flux-correction year (the original's own sequencing: each word gets its
own correction set).  The 16-run resolution-IV fraction over the eight bits -- free bits a = bit 4, b = bit 5,
c = bit 6, d = bit 3; generated bits 0 = a^b^c, 1 = a^b^d, 2 = a^c^d, 7 = b^c^d -- so every pair of bits meets in all
four states and every state of the three transport bits (4, 5, 6) occurs twice.

SET B, shared spin-up: the flux-correction year runs under word 0, the word is set after it (the engine un-shares the
correction sets) and one scenario year follows.  No word of it has NO_CIRCULATION: with corrections spun up under
circulation the model itself goes non-finite within a year for most such words.  Set B exists because bits 5 and 6 are
exactly invisible in set A wherever NO_HYDRO is set (the vapour is then decoupled and held on its corrected path).

The fixture tests/golden/switch_words_g96.npz is minted from the oracle (this project's own C restatement) alone.
"""
import os

import numpy as np

CO2 = 680.0
VARS = ("Tsurf", "Tair", "Tocean", "q", "albedo")
TOL = (1e-4, 1e-4, 1e-4, 2e-8, 1e-6)  # the project's whole-run tolerance (tests/test_gpu_logexp.py): RMS of a monthly-mean field


def _fraction():
    out = []
    for run in range(16):
        d, c, b, a = (run >> 3) & 1, (run >> 2) & 1, (run >> 1) & 1, run & 1
        bits = {4: a, 5: b, 6: c, 3: d, 0: a ^ b ^ c, 1: a ^ b ^ d, 2: a ^ c ^ d, 7: b ^ c ^ d}
        out.append(sum(v << k for k, v in bits.items()))
    return tuple(out)


SET_A = (0x00, 0x8e, 0xc5, 0x4b, 0xa3, 0x2d, 0x66, 0xe8, 0x17, 0x99, 0xd2, 0x5c, 0xb4, 0x3a, 0x71, 0xff)
SET_B = (0x08, 0x20, 0x40, 0x60, 0x29, 0x4c, 0xc8, 0xa2)
assert sorted(SET_A) == sorted(_fraction())
CASES = tuple(("a", w) for w in SET_A) + tuple(("b", w) for w in SET_B)
FIXTURE = "switch_words_g96.npz"


def key(which: str, word: int) -> str:
    return f"{which}_{word:02x}"


def oracle_case(O, inputs, params, which: str, word: int, years: int = 1):
    """The case on the oracle module O: (monthly [years][12][5][ny][nx], yearly [1 + years][2]: flux year, then scenario)."""
    o = O.Oracle(inputs, params)
    try:
        if which == "a":
            o.set_switches(word)
        yf = o.flux_correction(1)
        if which == "b":
            o.set_switches(word)
        mon, yr = o.run(years, CO2)
        return mon, np.concatenate([yf, yr])
    finally:
        o.close()


# ---- the fixture.  The 24 x 5 last-month fields are stored without loss but small enough to commit: a field that several
# cases share bit for bit (Tocean without deep ocean, albedo without ice, a masked transport bit) is stored once, and the
# float32 go as four byte planes (all lowest bytes, then all second bytes, ...): the same bits, but the planes of
# sign/exponent/high mantissa are nearly constant and deflate to almost nothing, which interleaved float32 do not.
def pack_f32(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, "<f4")
    return np.ascontiguousarray(a.view(np.uint8).reshape(-1, 4).T)


def unpack_f32(planes: np.ndarray, shape) -> np.ndarray:
    return np.ascontiguousarray(planes.T).view("<f4").reshape(shape).astype(np.float32, copy=False)


def pack_fields(last: np.ndarray):
    """last [n][5][ny][nx] -> (byte planes of the distinct fields, index [n][5] into them)."""
    seen, uniq, index = {}, [], np.empty(last.shape[:2], np.int32)
    for n in range(last.shape[0]):
        for v in range(last.shape[1]):
            b = last[n, v].tobytes()
            if b not in seen:
                seen[b] = len(uniq)
                uniq.append(last[n, v])
            index[n, v] = seen[b]
    return pack_f32(np.stack(uniq)), index


def load_fixture(golden_dir: str) -> dict:
    """{key: {"last" [5][ny][nx] f32, "means" [12][5] f64, "yearly" [2][2] f32, "sha256" bytes, "noise" [5] f64}}."""
    with np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False) as z:
        last = unpack_f32(z["fields_byteplanes"], (-1, 48, 96))[z["field_index"]]
        words = [(str(s), int(w)) for s, w in zip(z["case_set"], z["case_word"])]
        assert tuple(words) == CASES, "the fixture was minted for other word sets: run tests/golden/make_golden_switch_words.py"
        return {key(s, w): {"last": last[n], "means": z["means"][n], "yearly": z["yearly"][n],
                            "sha256": z["sha256"][n].tobytes(), "noise": z["noise"][n]} for n, (s, w) in enumerate(words)}


def bar(case: dict) -> np.ndarray:
    """[5]: max(TOL, 3 x the oracle's own sensitivity to contraction for this case)."""
    return np.maximum(np.asarray(TOL, np.float64), 3.0 * np.asarray(case["noise"], np.float64))
