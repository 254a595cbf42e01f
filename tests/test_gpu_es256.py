"""ES256 pass-signature verification on the device: the vectors of test_cpu_es256.py (built by es256_cases) through the
kernels of csrc/es256_verify.hip, the layer operator at the grid tails, device verdicts against the reference's and the
host route's, the verification schedule pinned in the exponent (es256_cases' families), and the relying party's
combined verdict for proofs of a 513-signal circuit."""
import pytest

import es256_cases as cases
import p256_ref as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_layer_ops_at_grid_tails(amd, count):
    cases.run_field_ops(amd, 0, count)
    cases.run_point_adds(amd, 0, count)
    cases.run_xcmp(amd, 0, count)


def test_signature_vectors(amd):
    cases.run_signature_cases(amd, 0)


def test_batch_of_130_over_three_keys(amd):
    keys, digests, sigs, idx, want = cases.batch130()
    amd.Es256Verifier(keys, device=0).close()   # a handle that never ran a batch
    dev, host = amd.Es256Verifier(keys, device=0), amd.Es256Verifier(keys, device=-1)
    assert dev.verify_batch(digests[:1], sigs[:1], idx[:1]) == host.verify_batch(digests[:1], sigs[:1], idx[:1])   # then it grows
    got = dev.verify_batch(digests, sigs, idx)
    assert got == want
    assert got == host.verify_batch(digests, sigs, idx)
    assert dev.verify_batch(digests[5:70], sigs[5:70], idx[5:70]) == host.verify_batch(digests[5:70], sigs[5:70], idx[5:70])
    assert [i for i, g in enumerate(got) if not g] == list(cases.BATCH_BAD)
    assert all(t >= 0 for t in dev.timings())
    dev.close()
    host.close()


def test_exceptional_sums_inside_a_wave(amd):
    keys, digests, sigs, idx, want = cases.mixed_wave()
    dev = amd.Es256Verifier(keys, device=0)
    assert dev.verify_batch(digests, sigs, idx) == want
    dev.close()


@pytest.mark.parametrize("family", "abcde")
def test_schedule_in_the_exponent(amd, family):
    """es256_cases' families (every table entry; equal, opposite and infinite operands at every key position of a lane and
    every slot of the shuffle tree; the compare's branches; scalar edges) at all four positions of a signature's lane
    group in its wavefront, dead groups among them: device verdicts against the construction's and the host route's"""
    batches = cases.exponent_batches(cases.EXPONENT_FAMILIES[family]())
    cases.run_exponent_batches(amd, 0, batches, rotations=(0, 1, 2, 3), against=-1)


def test_schedule_families_side_by_side(amd):
    """the families' concatenation: wavefronts that hold cases of two families, other cuts into batches and handles"""
    batches = cases.exponent_batches(cases.exponent_cases())
    cases.run_exponent_batches(amd, 0, batches, rotations=(0, 3))


def test_key_index_out_of_range(amd):
    digest, sig, _ = cases.golden_pass()
    dev = amd.Es256Verifier([cases.golden_key()], device=0)
    with pytest.raises(amd.G16Error) as e:
        dev.verify_batch([digest] * 2, [sig] * 2, [0, 1])
    assert e.value.code == -1 and "item 1" in str(e.value)
    dev.close()


# ------------------------------------------------------------------ the combined verdict
N_PUB, NOW = cases.N_PUB, cases.NOW


@pytest.fixture(scope="module")
def pass_circuit(amd):
    return cases.pass_circuit(amd)


def test_pass_proof_verdicts(amd, pass_circuit):
    vkey, pubs, proofs = pass_circuit
    _, sig, _ = cases.golden_pass()
    keys, sigcases = cases.signature_cases()
    foreign = next(c for c in sigcases if c[0] == "e = n + 5")   # a valid signature of key 1, but of another digest
    swapped = dict(proofs["a"], pi_c=proofs["c"]["pi_c"])
    ver = amd.Verifier(vkey, N_PUB, montgomery=True, device=0)
    es = amd.Es256Verifier(keys[:2], device=0)
    items = [("a", proofs["a"], sig, 0), ("a", proofs["a"], foreign[2], 1), ("c", proofs["c"], sig, 0),
             ("d", proofs["d"], sig, 0), ("a", swapped, sig, 0)]
    assert ver.verify_batch([(pubs[n], p) for n, p, _, _ in items]) == [True, True, True, True, False]
    got = amd.nzcp_pass_proof_verify(ver, es, [p for _, p, _, _ in items], [pubs[n] for n, _, _, _ in items],
                                     [s for _, _, s, _ in items], [k for _, _, _, k in items], now=NOW)
    assert got == [0, 3, 2, 4, 1]
    # now = 0 skips the expiry test; one item; none
    assert amd.nzcp_pass_proof_verify(ver, es, [proofs["d"]], [pubs["d"]], [sig]) == [0]
    assert amd.nzcp_pass_proof_verify(ver, es, [], [], []) == []
    ver.close()
    es.close()


def test_pass_proof_refusals(amd, pass_circuit):
    vkey, pubs, proofs = pass_circuit
    _, sig, _ = cases.golden_pass()
    ver = amd.Verifier(vkey, N_PUB, montgomery=True, device=0)
    host = amd.Es256Verifier([cases.golden_key()], device=-1)
    with pytest.raises(amd.G16Error) as e:
        amd.nzcp_pass_proof_verify(ver, host, [proofs["a"]], [pubs["a"]], [sig])
    assert e.value.code == -1 and "host route" in str(e.value)
    host.close()
    ver.close()
    _, _, small_vkey = amd.synth_setup(96, 5, 70, 11)
    small = amd.Verifier(small_vkey, 5, montgomery=True, device=0)
    es = amd.Es256Verifier([cases.golden_key()], device=0)
    with pytest.raises(amd.G16Error) as e:
        amd.nzcp_pass_proof_verify(small, es, [proofs["a"]], [[0] * 5], [sig])
    assert e.value.code == -1 and "513" in str(e.value)
    small.close()
    es.close()
