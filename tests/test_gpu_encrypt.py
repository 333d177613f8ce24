"""Sampling and encrypting on the device (sfp_sample_small: k_sample_small;
sfp_encrypt_combine: k_encrypt_combine) and the batched encrypt entry point.

Both samplers are integer functions of (seed, i), so the device path must give
the residues of the host path exactly: every comparison is `==` on the
downloaded residues (Ct.download()) of a `hip` and an `oracle` engine created
with the same seed -- the oracle has neither prim and samples on the host.
Their keys are compared too: the hip engine's public, relinearisation,
rotation and tier keys carry device-sampled errors.

Shapes, the smallest that reach every path: ring 2^11 (one k_ntt_small block
per row under sfp_ntt_batch), 2^12 and 2^13 (the two-pass NTT); depth 2 at
levels 0 and 2 (with the q_ext row R = 4 and R = 2 rows); FLEXIBLEAUTOEXT (the
ext row, the in-place combine and the division by q_ext) and FLEXIBLEAUTO (the
combine writes the ciphertext); 8 and n/2 slots; values of mixed sign with
magnitudes from 1e-3 to 255."""
import numpy as np
import pytest

import sfhe

pytestmark = pytest.mark.gpu

DEPTH = 2
RINGS = (11, 12, 13)
SCALINGS = ("FLEXIBLEAUTOEXT", "FLEXIBLEAUTO")
SEED = 90210


def mixed_values(rng, count):
    mag = 10.0 ** rng.uniform(-3.0, np.log10(255.0), count)
    return [float(x) for x in mag * rng.choice([-1.0, 1.0], count)]


def engine(backend, logn, scaling="FLEXIBLEAUTOEXT", **kw):
    return sfhe.Engine(backend, mult_depth=DEPTH, ring_dim=1 << logn, batch_size=8, seed=SEED + logn,
                       scaling=scaling, **kw)


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per (ring, scaling): a hip and an oracle engine with the same seed."""
    out = {(logn, sc): {b: engine(b, logn, sc) for b in ("hip", "oracle")} for logn in RINGS for sc in SCALINGS}
    yield out
    for eng in out.values():
        for e in eng.values():
            e.close()


@pytest.mark.parametrize("level", (0, DEPTH))
@pytest.mark.parametrize("full", (False, True), ids=("slots8", "slotsHalf"))
@pytest.mark.parametrize("scaling", SCALINGS)
@pytest.mark.parametrize("logn", RINGS)
def test_encrypt_bitexact_vs_oracle(pairs, monkeypatch, logn, scaling, full, level):
    monkeypatch.delenv("SFHE_DEV_SAMPLE", raising=False)
    eng = pairs[logn, scaling]
    slots = 1 << (logn - 1) if full else 8
    v = mixed_values(np.random.default_rng(1000 * logn + 10 * level + full), slots)
    cts = {}
    for b in ("hip", "oracle"):  # (both encrypt before anything is asserted: the shared engines' seeds stay in step)
        eng[b].op_stats(reset=True)
        cts[b] = eng[b].encrypt(v, slots, level)
    raw = {b: ct.download() for b, ct in cts.items()}
    for ct in cts.values():
        assert ct.info() == dict(level=level, slots=slots, limbs=DEPTH + 1 - level)
    bad = int(np.count_nonzero(raw["hip"] != raw["oracle"]))
    assert bad == 0, f"{bad} of {raw['hip'].size} residues differ from the host-sampled encryption"
    assert eng["hip"].sample_counts() == (3, 0)
    assert eng["oracle"].sample_counts() == (0, 3)


@pytest.mark.parametrize("scaling", SCALINGS)
def test_encrypt_batch_order(hip_lib, oracle_lib, monkeypatch, scaling):
    """Levels [0, 2, 0, 2, 0]: the level groups interleave in the list, the
    seeds may not."""
    monkeypatch.delenv("SFHE_DEV_SAMPLE", raising=False)
    logn, levels = 12, [0, DEPTH, 0, DEPTH, 0]
    rng = np.random.default_rng(5)
    inputs = [mixed_values(rng, 8) for _ in levels]
    hip, hip2, ora = engine("hip", logn, scaling), engine("hip", logn, scaling), engine("oracle", logn, scaling)
    hip.op_stats(reset=True)
    batch = hip.encrypt_batch(inputs, 8, levels)
    assert hip.sample_counts() == (3 * len(levels), 0)
    assert [c.level for c in batch] == levels
    for k, (v, lv) in enumerate(zip(inputs, levels)):
        got = batch[k].download()
        assert np.array_equal(got, ora.encrypt(v, 8, lv).download()), k
        assert np.array_equal(got, hip2.encrypt(v, 8, lv).download()), k
    # the seed counter advanced as five sequential encrypts advance it
    last = hip.encrypt(inputs[0], 8).download()
    assert np.array_equal(last, ora.encrypt(inputs[0], 8).download())
    assert np.array_equal(last, hip2.encrypt(inputs[0], 8).download())
    for e in (hip, hip2, ora):
        e.close()


def test_encrypt_batch_chunks(hip_lib, oracle_lib, monkeypatch):
    """More ciphertexts of one level than one launch set takes (64, context.cpp
    kEncryptChunk): 70 at level 0 and 3 at level 2, ring 2^11 -- the second
    chunk's seeds, scratch rows and outputs."""
    monkeypatch.delenv("SFHE_DEV_SAMPLE", raising=False)
    logn = 11
    levels = [0] * 40 + [DEPTH] * 3 + [0] * 30
    rng = np.random.default_rng(9)
    inputs = [mixed_values(rng, 8) for _ in levels]
    hip, ora = engine("hip", logn), engine("oracle", logn)
    hip.op_stats(reset=True)
    batch = hip.encrypt_batch(inputs, 8, levels)
    assert hip.sample_counts() == (3 * len(levels), 0)
    for k, (v, lv) in enumerate(zip(inputs, levels)):
        assert np.array_equal(batch[k].download(), ora.encrypt(v, 8, lv).download()), k
    hip.close()
    ora.close()


@pytest.mark.parametrize("logn", RINGS)
def test_knob_ab_in_one_process(hip_lib, monkeypatch, logn):
    a, b = engine("hip", logn), engine("hip", logn)
    rng = np.random.default_rng(logn)
    half = 1 << (logn - 1)
    jobs = [(mixed_values(rng, s), s, lv) for s in (8, half) for lv in (0, DEPTH)]
    monkeypatch.delenv("SFHE_DEV_SAMPLE", raising=False)
    a.op_stats(reset=True)
    dev = [a.encrypt(*j).download() for j in jobs]
    assert a.sample_counts() == (3 * len(jobs), 0)
    monkeypatch.setenv("SFHE_DEV_SAMPLE", "0")
    b.op_stats(reset=True)
    host = [b.encrypt(*j).download() for j in jobs]
    assert b.sample_counts() == (0, 3 * len(jobs))
    for k, (x, y) in enumerate(zip(dev, host)):
        assert np.array_equal(x, y), jobs[k][1:]
    a.close()
    b.close()


def test_keygen_samples_on_device(hip_lib, oracle_lib, monkeypatch):
    monkeypatch.delenv("SFHE_DEV_SAMPLE", raising=False)
    hip, ora = (engine(b, 12, rotations=[1, -1]) for b in ("hip", "oracle"))
    dev, host = hip.sample_counts()  # before any encrypt: the keys' errors (and the secret, on the host)
    assert dev > 0 and host == 1, (dev, host)
    assert ora.sample_counts() == (0, dev + host)
    v = mixed_values(np.random.default_rng(3), 8)
    ch, co = hip.encrypt(v, 8), ora.encrypt(v, 8)
    assert np.array_equal(ch.download(), co.download())  # the public key's error
    for r in (1, -1):  # the rotation keys' (and their tiers')
        assert np.array_equal(hip.rotate(ch, r).download(), ora.rotate(co, r).download()), r
    assert np.array_equal(hip.mult(ch, ch).download(), ora.mult(co, co).download())  # the relinearisation key's
    hip.close()
    ora.close()


@pytest.mark.parametrize("logn", RINGS)
def test_roundtrip(pairs, monkeypatch, logn):
    monkeypatch.delenv("SFHE_DEV_SAMPLE", raising=False)
    e = pairs[logn, "FLEXIBLEAUTOEXT"]["hip"]
    half = 1 << (logn - 1)
    v = mixed_values(np.random.default_rng(40 + logn), half)
    got = np.array(e.decrypt(e.encrypt(v, half)))
    assert got.shape == (half,)
    assert float(np.max(np.abs(got - np.array(v)))) < 1e-4
