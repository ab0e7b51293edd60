"""CPU checks of the resamplers: the C ABI declares and exports them and the mirror binds them, every refusal of a table is one in the
library's own check, in the Python mirror and in the restatement, the host helpers compute what the header states, the NumPy
restatement (tests/resample_ref.py) agrees with the samplers' linear and nearest values through tables that say the same, holds the split
law, and orders of summation other than the stated one show -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resample_ref as ref
import sampler_ref as sref
import voice_ref as vref
from oalsfxpp_amd import api, lib
from test_sampler_abi import rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oalsfx_batch_set_fir_table", "oalsfx_batch_get_fir_table", "oalsfx_batch_set_resamplers", "oalsfx_batch_get_resamplers")
HOST_NAMES = ("oalsfx_host_fir_check", "oalsfx_host_fir_sinc", "oalsfx_host_fir_cubic")
f32 = np.float32
ONE = sref.ONE


def test_header_declares_and_the_mirror_binds_the_resampler_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES + HOST_NAMES[:2]:
        assert re.search(r"\bint " + name + r"\(", header), name
    assert re.search(r"\bvoid oalsfx_host_fir_cubic\(", header)
    assert header.index("---- resamplers") > header.index("---- voice envelopes")
    assert re.search(r"#define OALSFX_FIR_TABLES 8\b", header) and re.search(r"#define OALSFX_RESAMPLER_NONE \(-1\)", header)
    debug = open(os.path.join(ROOT, "include", "oalsfx_hip_debug.h")).read()
    assert re.search(r"\blong long oalsfx_debug_resampler_uploads\(", debug) and '"k_fir_rows"' in debug
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES + HOST_NAMES + ("oalsfx_debug_resampler_uploads",):
        assert name in lib.SIGNATURES and hasattr(so, name), name
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("phase = (q & 4095) >> (12 - phase_bits)", "j_k = i - (H - 1) + k", "loop_start + (j_k - loop_end) mod (loop_end - loop_start)",
                   "the lead-in is read where it lies", "v = (((+0.0f + c_0 * x_0) + c_1 * x_1) + ...) + c_(T-1) * x_(T-1)", "no fused multiply-add",
                   "An in-range tap is always multiplied, even by a zero coefficient", "An out-of-range tap may be multiplied or left out",
                   "The sampler's LINEAR flag is not looked at", "an out-of-range tap is never loaded",
                   "oalsfx_batch_reset, _snapshot and _restore neither touch nor carry them"):
        assert phrase in flat, phrase
    for method in ("set_fir_table", "get_fir_table", "set_resamplers", "get_resamplers", "resampler_uploads"):
        assert callable(getattr(api.Batch, method))
    assert callable(api.fir_cubic) and callable(api.fir_sinc) and api.FIR_TABLES == ref.FIR_TABLES == 8 and api.RESAMPLER_NONE == ref.NONE == -1
    array = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    assert re.search(r"bool set_fir_table\(int table, int taps, int phase_bits, const float\* coef\);", array)
    assert re.search(r"bool set_resampler\(int index, int table\);", array) and re.search(r"bool get_resampler\(int index, int& table\);", array)
    kernel = open(os.path.join(ROOT, "oalsfxpp_amd", "csrc", "hip", "resample.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "__shared__" not in kernel and "k_sampler_" not in kernel


# ---- refusals: the library's check, the Python mirror and the restatement say the same ----
def _table(taps, phase_bits, fill=0.25):
    return np.full(((1 << phase_bits), taps), fill, f32)


def _with(table, at, value):
    table = table.copy()
    table.reshape(-1)[at] = value
    return table


REFUSALS = [
    (0, 0, _table(4, 0), "Unknown FIR tap count."), (2, 4, _table(4, 4), "Unknown FIR tap count."), (16, 4, _table(8, 5), "Unknown FIR tap count."),
    (-4, 4, _table(4, 4), "Unknown FIR tap count."), (6, 4, _table(8, 4), "Unknown FIR tap count."),
    (4, -1, _table(4, 0), "FIR phase bits out of range."), (8, 13, _table(8, 12), "FIR phase bits out of range."),
    (4, 3, None, "Null FIR coefficients."), (8, 0, None, "Null FIR coefficients."),
    (4, 0, _with(_table(4, 0), 3, np.nan), "Non-finite FIR coefficient."), (8, 12, _with(_table(8, 12), 8 * 4096 - 1, np.inf), "Non-finite FIR coefficient."),
    (4, 5, _with(_table(4, 5), 17, -np.inf), "Non-finite FIR coefficient."),
    (3, 13, None, "Unknown FIR tap count."), (4, 13, None, "FIR phase bits out of range.")]          # the order of the checks


@pytest.mark.parametrize("taps, phase_bits, coef, message", REFUSALS)
def test_a_table_is_refused(taps, phase_bits, coef, message):
    assert api.fir_check(taps, phase_bits, coef) == message
    assert ref.check(taps, phase_bits, coef) == message
    if coef is not None and phase_bits >= 0 and coef.shape == (1 << phase_bits, taps):
        with pytest.raises(api.BatchError, match=re.escape(message)):
            api.fir_shape(coef)


def test_tables_that_are_taken_and_what_the_mirror_refuses_by_shape():
    for taps in (4, 8):
        for bits in range(13):
            t = _table(taps, bits, fill=-3e38)
            assert api.fir_check(taps, bits, t) is None and ref.check(taps, bits, t) is None and api.fir_shape(t) == (taps, bits)
    denormal = _with(_table(4, 2), 5, 1e-45)
    assert api.fir_check(4, 2, denormal) is None and ref.check(4, 2, denormal) is None
    for bad, message in ((np.zeros((3, 4), f32), "FIR phase bits out of range."), (np.zeros((8192, 4), f32), "FIR phase bits out of range."),
                         (np.zeros((4, 5), f32), "Unknown FIR tap count."), (np.zeros(16, f32), "Unknown FIR tap count."), (None, "Null FIR coefficients.")):
        with pytest.raises(api.BatchError, match=re.escape(message)):
            api.fir_shape(bad)
    unopened = api.Batch.__new__(api.Batch)
    unopened.n, unopened.channels, unopened._h, unopened._lib = 8, 2, None, None
    for table in (-1, 8):
        with pytest.raises(api.BatchError, match="FIR table index out of range."):
            unopened.set_fir_table(table, _table(4, 0))
    with pytest.raises(api.BatchError, match="Non-finite FIR coefficient."):
        unopened.set_fir_table(0, _with(_table(4, 1), 0, np.nan))
    for tables in ([-2], [8], [0, 1, 99]):
        with pytest.raises(api.BatchError, match="Unknown resampler."):
            unopened.set_resamplers(tables, instances=list(range(len(tables))))
    with pytest.raises(api.BatchError, match="listed twice"):
        unopened.set_resamplers([0, 0], instances=[1, 1])
    with pytest.raises(api.BatchError, match="out of bounds"):
        unopened.set_resamplers([0] * 9)


# ---- the host helpers ----
@pytest.mark.parametrize("bits", [0, 1, 8, 12])
def test_cubic_is_the_restatement_on_its_bits(bits):
    got, want = api.fir_cubic(bits), ref.cubic(bits)
    assert got.shape == (1 << bits, 4) and sref.same_bits(got, want)
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22 and (got[0] == [0, 1, 0, 0]).all()
    # Horner's form gives the same values (every term is exact in double with at most 12 bits in mu), and the same bits but for the sign
    # of the zeros at mu = 0, which the power form the header states leaves positive
    mu = np.arange(1 << bits, dtype=np.float64) / (1 << bits)
    horner = np.stack([((-0.5 * mu + 1.0) * mu - 0.5) * mu, (1.5 * mu - 2.5) * mu * mu + 1.0, ((-1.5 * mu + 2.0) * mu + 0.5) * mu, (0.5 * mu - 0.5) * mu * mu], axis=1)
    assert (horner.sum(axis=1) == 1.0).all(), "every row sums to 1 in double"
    assert (got == horner.astype(f32)).all() and sref.same_bits(got[1:], horner.astype(f32)[1:]) and not np.signbit(got[0]).any()


@pytest.mark.parametrize("cutoff", [1.0, 0.5, 0.37, 4096 / 5793])
@pytest.mark.parametrize("bits", [0, 3, 8, 12])
@pytest.mark.parametrize("taps", [4, 8])
def test_sinc_is_the_formula(taps, bits, cutoff):
    got, want = api.fir_sinc(taps, bits, cutoff), ref.sinc_double(taps, bits, cutoff)
    P = 1 << bits
    assert got.shape == (P, taps) and got.dtype == f32 and np.isfinite(got).all()
    # both sides round a double of magnitude <= 1 to float once; libm may move that double by an ulp: one float ulp at the most, 2^-23
    # below 1 -- and 2^-22 is the bound
    assert np.abs(want).max() <= 1.0 and np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -22
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
    # the phases p and P - p mirror each other: tap k of one is at the distance of tap T - 1 - k of the other, with the other sign
    p = np.arange(1, P)
    assert sref.same_bits(got[p], got[P - p][:, ::-1])
    assert api.fir_check(taps, bits, got) is None
    if cutoff == 1.0:
        # at phase 0 and the full band the filter is the sample itself, but for sin(pi k) not being 0 in double
        assert np.abs(got[0] - ref.nearest_table(0, taps)[0]).max() < 1e-15


def test_sinc_refuses_its_arguments():
    so = lib.load()
    out = np.full(64, 7.0, f32)
    for taps, bits, cutoff in ((6, 2, 0.5), (4, -1, 0.5), (4, 13, 0.5), (8, 2, 0.0), (8, 2, -0.5), (8, 2, 1.0000001), (8, 2, np.nan)):
        assert so.oalsfx_host_fir_sinc(taps, bits, cutoff, C.c_void_p(out.ctypes.data)) == 0 and (out == 7.0).all()
    with pytest.raises(api.BatchError):
        api.fir_sinc(4, 2, 0.0)
    with pytest.raises(api.BatchError):
        api.fir_cubic(13)


# ---- the restatement against the samplers' contract ----
def _cases(rng, count, channels):
    from test_sampler_abi import random_records
    return random_records(rng, count, channels, assets_per_format=2, asset_frames=(1, 400))


def test_the_linear_and_the_nearest_table_say_what_the_samplers_say():
    rng = np.random.default_rng(31)
    q_all = rng.integers(0, 2 ** 40, 3000).astype(np.uint64)
    checked = 0
    for channels in (1, 2, 6):
        records, pcm, _, _ = _cases(rng, 120, channels)
        for r, asset in zip(records, pcm):
            limit = int(r["loop_end"] if int(r["flags"]) & sref.LOOP else r["frames"]) << sref.FRAC_BITS
            q = q_all % np.uint64(limit)
            nearest, linear = r.copy(), r.copy()
            nearest["flags"] = int(r["flags"]) & ~sref.LINEAR
            linear["flags"] = int(r["flags"]) | sref.LINEAR
            for bits in (12, 0):
                got, live = ref.values(r, asset, q, channels, ref.nearest_table(bits))
                want, live_too = vref.values(nearest, asset, q, channels)
                assert (live == live_too).all() and sref.same_floats(got, want)[0], "the nearest-sample table"
            got, _ = ref.values(r, asset, q, channels, ref.linear_table(12))
            want, _ = vref.values(linear, asset, q, channels)
            # the samplers' a + ((b - a) * mu) has three roundings, the table's (0 + (1 - mu) a) + mu b four (1 - mu is exact), each at
            # most 2^-24 of a magnitude no larger than |a| + |b|; the gain's rounding adds one relative 2^-24 to each side
            i = (q >> np.uint64(12)).astype(np.int64)
            x, _ = ref.taps_of(r, asset, i, np.ones(len(q), bool), 4)
            scale = np.abs(x[:, 1]) + np.abs(x[:, 2])
            if int(r["channels"]) == 1:
                scale = np.repeat(scale, channels, axis=1)
            bound = 10.0 * 2.0 ** -24 * scale.astype(np.float64) * np.abs(r["gain"][:channels]).astype(np.float64)[None, :] + 1e-45
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound).all(), "the linear table"
            checked += 1
    assert checked == 360


def _random_cases(rng, count, channels, enveloped):
    """`count` (record, envelope, table or None, asset): a third each at 4 taps, at 8 taps and without a table."""
    tables = {0: ref.cubic(12), 1: ref.sinc(8, 12, 0.8), 2: ref.sinc(4, 3, 0.5), 3: ref.sinc(8, 0, 1.0), 4: ref.linear_table(7)}
    if enveloped:
        records, envelopes, pcm, _, _ = vref.random_pairs(rng, count, channels, assets_per_format=2, asset_frames=(1, 400))
    else:
        records, pcm, _, _ = _cases(rng, count, channels)
        envelopes = np.zeros(count, vref.DTYPE)
    resamplers = np.asarray([(0, 1, ref.NONE, 2, 3, ref.NONE, 4, 1, ref.NONE)[r % 9] for r in range(count)])
    return records, envelopes, resamplers, tables, pcm


@pytest.mark.parametrize("enveloped", [False, True])
def test_any_split_of_a_call_gives_the_same_outputs_and_records(enveloped):
    rng = np.random.default_rng(40 + enveloped)
    records, envelopes, resamplers, tables, pcm = _random_cases(rng, 1000, 2, enveloped)
    whole, after, env_after = ref.render(records, envelopes, resamplers, tables, pcm, sum(vref.CALLS), 2)
    state, env_state, parts = records, envelopes, []
    for frames in vref.CALLS:
        out, state, env_state = ref.render(state, env_state, resamplers, tables, pcm, frames, 2)
        parts.append(out)
    assert sum(vref.CALLS) == 2500 and vref.CALLS == (441, 256, 1, 1802)
    assert sref.same_floats(np.concatenate(parts, axis=1), whole)[0]
    assert state.tobytes() == after.tobytes() and env_state.tobytes() == env_after.tobytes()
    assert np.abs(whole).max() > 0 and (after["position"] != records["position"]).any()
    # without a table the restatement is the envelopes', and without an envelope the samplers'
    plain = [r for r in range(1000) if resamplers[r] == ref.NONE]
    theirs, after_theirs, _ = vref.render(records[plain], envelopes[plain], [pcm[r] for r in plain], 2500, 2)
    assert sref.same_floats(whole[plain], theirs)[0] and after[plain].tobytes() == after_theirs.tobytes()


# ---- the order of the sum shows ----
def _stated(c, x):
    return ref.fir(c, x[:, :, None])[:, 0]


def _descending(c, x):
    return ref.fir(c[:, ::-1], x[:, ::-1, None])[:, 0]


def _fused(c, x):
    """A chain of fused multiply-adds in ascending order: the product of two floats is exact in double, and the sum is rounded once to
    float (through double, which differs from a true fma only where the double sum lies within 2^-29 ulp of a float tie)."""
    v = np.zeros(len(x), f32)
    for k in range(x.shape[1]):
        v = (c[:, k].astype(np.float64) * x[:, k].astype(np.float64) + v.astype(np.float64)).astype(f32)
    return v


def _pairwise(c, x):
    """A tree: neighbours first."""
    p = [c[:, k] * x[:, k] for k in range(x.shape[1])]
    while len(p) > 1:
        p = [p[k] + p[k + 1] for k in range(0, len(p), 2)]
    return p[0]


SHARES = {}


@pytest.mark.parametrize("kind", ["s16", "f32"])
@pytest.mark.parametrize("taps", [4, 8])
def test_another_order_of_the_sum_shows(taps, kind):
    """2^20 random phases and samples: a descending order, a fused chain and a pairwise tree each differ from the stated value in at least
    a tenth of the outputs (measured: DESIGN.md 4g), so a kernel that took one of them would not pass the comparisons on the bits."""
    rng = np.random.default_rng(taps + (kind == "f32"))
    n = 1 << 20
    table = ref.cubic(12) if taps == 4 else ref.sinc(8, 12, 0.9)
    c = table[rng.integers(0, 4096, n)]
    if kind == "s16":
        x = sref.to_float(rng.integers(-32768, 32768, (n, taps)).astype(np.int16))
    else:
        x = rng.standard_normal((n, taps)).astype(f32)
    want = _stated(c, x)
    for name, variant in (("descending", _descending), ("fused", _fused), ("pairwise", _pairwise)):
        got = variant(c, x)
        share = float((got.view(np.uint32) != want.view(np.uint32)).mean())
        SHARES[(taps, kind, name)] = share
        print(f"T = {taps}, {kind}, {name}: {100 * share:.1f} % of the outputs differ")
        assert share >= 0.10, (taps, kind, name, share)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -20 * np.abs(x).max() * taps, "a variant is the same sum up to rounding"
