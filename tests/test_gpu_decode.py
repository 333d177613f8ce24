"""Decoding on the device at the end of a decryption (sfp_decode_batch: the
k_dec_load / k_dec_tile / k_dec_stage kernels).

The contract is bit identity with the host decoder (the CRT lift and centring
of CryptoContextImpl::Decrypt followed by core/encoder.cpp ckks_decode), so
every comparison is exact.  The same ciphertexts are built on `hip` and on
`oracle` with the same seed (the parity tests establish equal residues); the
oracle decodes on the host.  Shapes: the smallest that reach every path --
no stage (1 slot), sparse packings, exactly one LDS tile (2048 slots), and
two tiles = n/2 at ring 2^13 (one global stage, gap 1) -- each at level 0
(two limbs: the 120-bit lift) and at the last level (one limb), with negative
entries and magnitudes from 1e-3 to 255 (both centring branches, many
exponents)."""
import numpy as np
import pytest

import sfhe
from oracle import slotsim

pytestmark = pytest.mark.gpu

DEPTH = 2
TILE = 2048  # csrc/hip/prims_hip.hip kEncTile
SHAPES = {12: [1, 2, 8, TILE], 13: [8, TILE, 2 * TILE]}
CASES = [(logn, slots, level) for logn, sl in SHAPES.items() for slots in sl for level in (0, DEPTH)]


def mixed_values(rng, count):
    mag = 10.0 ** rng.uniform(-3.0, np.log10(255.0), count)
    return [float(x) for x in mag * rng.choice([-1.0, 1.0], count)]


@pytest.fixture(scope="module")
def rings(hip_lib, oracle_lib):
    """Per ring: the hip engine, its ciphertexts by (slots, level), and the
    oracle's decryptions of the same ciphertexts (computed once)."""
    out = {}
    for logn, shapes in SHAPES.items():
        assert max(shapes) == 1 << (logn - 1)  # the full packing (gap 1) of each ring is among them
        eng = {b: sfhe.Engine(b, mult_depth=DEPTH, ring_dim=1 << logn, batch_size=8, seed=777 + logn)
               for b in ("hip", "oracle")}
        rng = np.random.default_rng(logn)
        cts, ref = {}, {}
        for slots in shapes:
            for level in (0, DEPTH):
                v = mixed_values(rng, slots)
                cts[slots, level] = eng["hip"].encrypt(v, slots, level)
                ref[slots, level] = np.array(eng["oracle"].decrypt(eng["oracle"].encrypt(v, slots, level)))
                assert np.allclose(ref[slots, level], v, rtol=0, atol=1e-4)
        eng["oracle"].close()
        out[logn] = (eng["hip"], cts, ref)
    yield out
    for e, _, _ in out.values():
        e.close()


@pytest.mark.parametrize("logn,slots,level", CASES)
def test_decrypt_bitexact_vs_oracle(rings, monkeypatch, logn, slots, level):
    monkeypatch.delenv("SFHE_DEV_DECODE", raising=False)
    e, cts, ref = rings[logn]
    ct = cts[slots, level]
    assert ct.info()["limbs"] == (1 if level == DEPTH else DEPTH + 1)
    e.op_stats(reset=True)
    got = np.array(e.decrypt(ct))
    assert e.decode_counts() == (1, 0)
    bad = int(np.count_nonzero(got != ref[slots, level]))
    assert bad == 0, f"{bad} of {slots} slots differ from the host decoder"


@pytest.mark.parametrize("logn", sorted(SHAPES))
def test_knob_ab_in_one_process(rings, monkeypatch, logn):
    e, cts, ref = rings[logn]
    keys = sorted(cts)
    monkeypatch.delenv("SFHE_DEV_DECODE", raising=False)
    e.op_stats(reset=True)
    dev = [np.array(e.decrypt(cts[k])) for k in keys]
    d1, h1 = e.decode_counts()
    assert d1 >= 1 and h1 == 0, (d1, h1)
    monkeypatch.setenv("SFHE_DEV_DECODE", "0")
    host = [np.array(e.decrypt(cts[k])) for k in keys]
    d2, h2 = e.decode_counts()
    assert d2 == d1 and h2 == len(keys), (d1, h1, d2, h2)
    for k, a, b in zip(keys, dev, host):
        assert np.array_equal(a, b), k
        assert np.array_equal(b, ref[k]), k


@pytest.mark.parametrize("logn", sorted(SHAPES))
def test_decrypt_batch_mixed(rings, monkeypatch, logn):
    monkeypatch.delenv("SFHE_DEV_DECODE", raising=False)
    e, cts, ref = rings[logn]
    keys = sorted(cts)[::-1] + sorted(cts)[:3]  # every (slots, level), some twice, groups interleaved
    lst = [cts[k] for k in keys]
    single = [np.array(e.decrypt(c)) for c in lst]
    e.op_stats(reset=True)
    batch = e.decrypt_batch(lst)
    assert e.decode_counts() == (len(lst), 0)
    assert [len(v) for v in batch] == [k[0] for k in keys]
    for k, a, b in zip(keys, single, batch):
        assert np.array_equal(a, np.array(b)), k
        assert np.array_equal(a, ref[k]), k


def test_debug_sort_prints_the_same(hip_lib, capfd, monkeypatch):
    """A DirectSort<8> debug sorter (the PRINT_PT decrypts inside sort()):
    the same text and the same residues with the decoding on the host and on
    the device."""
    N, logn = 8, 12
    depth, rots = sfhe.direct_sort_params(N, "hip")
    e = sfhe.Engine("hip", mult_depth=depth, ring_dim=1 << logn, batch_size=N, rotations=rots, seed=20251205 + N)
    cfg = slotsim.default_sign_config(N)
    s = e.sorter(N, debug=True)
    ct = e.encrypt(slotsim.input_vector(N).tolist())
    s.sort(ct, *cfg)  # (the first sort sees its input at N slots: text differs)
    e.sync()
    res = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SFHE_DEV_DECODE", knob)
        e.op_stats(reset=True)
        capfd.readouterr()
        raw = s.sort(ct, *cfg).download()
        e.sync()
        res[knob] = (capfd.readouterr().out, raw, e.decode_counts())
    (t0, r0, c0), (t1, r1, c1) = res["0"], res["1"]
    assert "Constructed Rank" in t0 and "Final Output" in t0
    assert c0[0] == 0 and c0[1] >= 3, c0
    assert c1[1] == 0 and c1[0] == c0[1], (c0, c1)
    assert t0 == t1
    assert np.array_equal(r0, r1)
    e.close()
