"""Pass verification from URIs on the device (device 0): the cases of test_cpu_pass.py through the front-end kernel and
the ES256 kernels behind it, record by record against pass_ref; and the ES256 entry point after a pass batch.  Every
input given to the device here has been cleared on the host by test_cpu_pass.py's sanitizer run or is a builder case."""
import pytest

import es256_cases
import pass_cases as cases

pytestmark = pytest.mark.gpu
DEV = 0


def test_example_pass(amd):
    cases.run_example(amd, DEV)


def test_sha256_padding_edges(amd):
    cases.run_sha256_edges(amd, DEV)


def test_full_call_padding_edges(amd):
    cases.run_cases(amd, DEV, cases.padding_cases())


def test_base32_tails(amd):
    cases.run_base32_tails(amd, DEV)


def test_cbor_heads(amd):
    cases.run_cases(amd, DEV, cases.cbor_cases())


def test_front_end_operator(amd):
    cases.run_front_op(amd, DEV)


def test_verdict_precedence(amd):
    cases.run_cases(amd, DEV, cases.precedence_cases())


def test_uri_cap(amd):
    cases.run_cases(amd, DEV, cases.cap_cases())


def test_grid_tails(amd):
    cases.run_grid_tails(amd, DEV)


def test_whole_corpus(amd):
    cases.run_corpus(amd, DEV)


def test_errors(amd):
    cases.run_errors(amd, DEV)


def test_es256_entry_point_after_a_pass_batch(amd):
    """g16_es256_verify_batch gives its verdicts as before once the process has run the pass route"""
    uris, records = cases.corpus()
    assert cases.run_batch(amd, DEV, uris[:65]) == records[:65]
    es256_cases.run_signature_cases(amd, DEV)
    keys, digests, sigs, idx, want = es256_cases.batch130()
    v = amd.Es256Verifier(keys, device=DEV)
    assert v.verify_batch(digests, sigs, idx) == want
    v.close()
