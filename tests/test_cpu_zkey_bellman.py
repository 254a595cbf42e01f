"""CPU side of the phase-2 MPCParams exchange (csrc/zkey_bellman_host.cpp): the Python twin (tests/zkey_bellman_ref.py)
against the closed form of H in pure Python, and every refusal and format error the host reaches before the device --
lengths, flags, a coordinate >= q, counts, csHash, records -- each with its own text and ahead of G16_E_NOGPU."""
import struct

import pytest

import bn254 as b
import formats as f
import groth16 as g
import synth
import zkey_bellman_ref as ref
import zkey_mpc_ref as mref
from bn254 import Q, R

TD = {"tau": 0x1234567 ** 5 % R, "alpha": 0xabcdef ** 7 % R, "beta": 0x55aa ** 11 % R, "gamma": 1, "delta": 1}
D, S = 0x1f2e3d4c5b6a7988 ** 3 % R, 0x0123456789abcdef ** 3 % R
FORMAT = "mpcparams: Invalid File format"


def _gpu_present(amd):
    """The library's own answer: the smallest device call there is (one point, the twist alone)."""
    try:
        amd.zkey_h_basis(bytes(64), 0)
    except amd.G16Error as e:
        if e.code == -4:
            return False
        raise
    return True


# ------------------------------------------------------------------ the twin against the closed form
def _s9(tau, L, delta=1):
    N = 1 << L
    lag = g.lagrange_at(2 * N, tau)
    dinv = pow(delta, -1, R)
    return [lag[2 * i + 1] * dinv % R for i in range(N)]


@pytest.mark.parametrize("L", [0, 1, 2, 3])
@pytest.mark.parametrize("tau", [TD["tau"], 5, R - 2])
def test_forward_of_section_9_is_the_monomial_basis(L, tau):
    N, delta = 1 << L, 77
    t = ref.basis_forward(_s9(tau, L, delta), L)
    z = (pow(tau, N, R) - 1) * pow(delta, -1, R) % R
    assert t == [pow(tau, k, R) * z % R for k in range(N)]       # every k, N - 1 included
    assert t[N - 1] != 0
    assert t[:N - 1] == ref.h_closed_form(tau, N, delta)


@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_inverse_undoes_forward_and_the_projection_is_idempotent(L):
    N = 1 << L
    a = [pow(3 + i, 50 + i, R) for i in range(N)]
    assert ref.basis_inverse(ref.basis_forward(a, L), L) == a
    assert ref.basis_forward(ref.basis_inverse(a, L), L) == a
    p = ref.project(a, L)
    assert ref.project(p, L) == p
    assert ref.basis_forward(p, L)[-1] == 0
    if L:
        assert p != a


@pytest.mark.parametrize("L", [1, 2, 3])
def test_projection_keeps_every_quotient_of_degree_n_minus_2(L):
    """sum e_i S9[i] with e_i = h(w^(2i+1)), deg h <= N - 2: what a prover forms from section 9."""
    N, w = 1 << L, b.fr_root(L + 1)
    a = _s9(TD["tau"], L)
    p = ref.project(a, L)
    h = [pow(7 + k, 30 + k, R) for k in range(N - 1)]
    e = [sum(c * pow(w, (2 * i + 1) * k, R) for k, c in enumerate(h)) % R for i in range(N)]
    assert sum(x * y for x, y in zip(e, a)) % R == sum(x * y for x, y in zip(e, p)) % R
    top = [pow(w, (2 * i + 1) * (N - 1), R) for i in range(N)]   # degree N - 1: NOT kept
    assert sum(x * y for x, y in zip(top, a)) % R != sum(x * y for x, y in zip(top, p)) % R


def test_points_and_images_round_trip():
    pts = ref.points([0, 1, 2, R - 1])
    assert pts[:64] == bytes(64) and pts[64:128] == f.g1_to_lem(b.G1_GEN)
    be = ref.run_be(pts, 64)
    assert be[:64] == ref.G1_INF_BE and be[64:128] == (1).to_bytes(32, "big") + (2).to_bytes(32, "big")
    assert b"".join(ref.g1_from_be(be[i:i + 64]) for i in range(0, 256, 64)) == pts
    for bad in (bytes([0x80]) + be[65:128], bytes([0x40, 1]) + bytes(62), Q.to_bytes(32, "big") + be[96:128], be[64:96] + be[64:96]):
        with pytest.raises(ValueError):
            ref.g1_from_be(bad)


# ------------------------------------------------------------------ the host's refusals
@pytest.fixture(scope="module")
def key(amd):
    n, p, m, seed = 24, 2, 12, 1
    _, rows, _ = synth.gen_circuit(n, p, m, seed)
    zkey, _ = amd.r1cs_setup_trapdoor(f.write_r1cs(n, p, 0, rows), TD, 2)
    return zkey


@pytest.fixture(scope="module")
def challenge(key):
    """The twin's MPCParams image of the key, H from the closed form (tau is known)."""
    sec = ref.key_sections(key)
    N = struct.unpack_from("<I", sec[2], 80)[0]
    assert N == 16 and len(sec[9]) == 64 * N
    return ref.write_mpcparams(sec, ref.run_be(ref.points(ref.h_closed_form(TD["tau"], N)), 64))


@pytest.fixture(scope="module")
def response(key, challenge):
    """The challenge with one record more, written by the twin (H and L left as they are: the host checks below never
    look at them)."""
    _, s10, _ = mref.contribute_ref(key, None, D, S)
    _, recs = mref.parse_section10(s10)
    m = ref.parse_mpcparams(challenge)
    at = m["at"]["csHash"]
    return challenge[:at + 64] + struct.pack(">I", 1) + ref.record_be(recs[0])


def _err(amd, call):
    with pytest.raises(amd.G16Error) as e:
        call()
    return e.value


def _patch(buf, at, data):
    return buf[:at] + data + buf[at + len(data):]


def _malformed(challenge):
    m = ref.parse_mpcparams(challenge)
    at = m["at"]
    a0 = at["A"] + 4
    out = {
        "empty": b"", "header_only": challenge[:ref.HEADER], "truncated": challenge[:-1], "trailing": challenge + b"\0",
        "count_without_points": _patch(challenge, at["L"], struct.pack(">I", len(m["L"]) // 64 + 1)),
        "record_count": _patch(challenge, at["csHash"] + 64, struct.pack(">I", 1)),
        "flag_0x80": _patch(challenge, a0, bytes([challenge[a0] | 0x80])),
        "flag_0x40_on_a_point": _patch(challenge, a0, bytes([challenge[a0] | 0x40])),
        "flag_both": _patch(challenge, a0, bytes([0xc0]) + bytes(63)),
        "x_is_q": _patch(challenge, a0, Q.to_bytes(32, "big")),
        "y_is_q": _patch(challenge, at["IC"] + 4 + 32, Q.to_bytes(32, "big")),
        "g2_c0_above_q": _patch(challenge, at["B2"] + 4 + 32, (Q + 1).to_bytes(32, "big")),
        "header_beta2_is_q": _patch(challenge, 128 + 64, Q.to_bytes(32, "big")),
    }
    return out


@pytest.mark.parametrize("what", ["empty", "header_only", "truncated", "trailing", "count_without_points", "record_count",
                                  "flag_0x80", "flag_0x40_on_a_point", "flag_both", "x_is_q", "y_is_q", "g2_c0_above_q",
                                  "header_beta2_is_q"])
def test_a_malformed_file_is_a_format_error_in_both_readers(amd, key, challenge, what):
    bad = _malformed(challenge)[what]
    e = _err(amd, lambda: amd.zkey_bellman_contribute(bad, D, S, device=0))
    assert e.code == -2 and str(e) == FORMAT
    e = _err(amd, lambda: amd.zkey_import_bellman(key, bad, "x", device=0))
    assert e.code == -2 and str(e) == FORMAT


def test_contribute_refuses_bad_secrets_and_deltas(amd, challenge):
    for d, s in ((0, S), (D, 0), (R, S), (D, R + 1)):
        e = _err(amd, lambda: amd.zkey_bellman_contribute(challenge, d, s, device=0))
        assert e.code == -1 and str(e) == "zkey bellman contribute: the secret scalars must be in [1, r)"
    with pytest.raises(ValueError):
        amd.zkey_bellman_contribute(challenge, D, None)
    inf = _patch(challenge, ref.DELTA1, ref.G1_INF_BE)
    off = _patch(challenge, ref.DELTA1 + 32, (5).to_bytes(32, "big"))
    for bad in (inf, off):
        e = _err(amd, lambda: amd.zkey_bellman_contribute(bad, D, S, device=0))
        assert e.code == -2 and str(e) == FORMAT


def _verdict(amd, key, resp, text):
    e = _err(amd, lambda: amd.zkey_import_bellman(key, resp, "x", device=0))
    assert e.code == 0 and str(e) == "zkey import bellman: " + text


def test_import_verdicts_of_the_host(amd, key, challenge, response):
    m = ref.parse_mpcparams(response)
    at = m["at"]
    # a count that is not the key's: one A point less, the file still consistent with itself
    fewer = response[:at["A"]] + struct.pack(">I", len(m["A"]) // 64 - 1) + m["A"][64:] + response[at["B1"]:]
    _verdict(amd, key, fewer, "a count is not the key's")
    no_h = response[:at["H"]] + struct.pack(">I", 0) + response[at["L"]:]
    _verdict(amd, key, no_h, "a count is not the key's")
    # alpha1 replaced by beta1
    _verdict(amd, key, _patch(response, 0, response[64:128]), "alpha, beta, gamma, IC, A, B1 or B2 differ from the key's")
    _verdict(amd, key, _patch(response, 256, response[128:256]), "alpha, beta, gamma, IC, A, B1 or B2 differ from the key's")
    _verdict(amd, key, _patch(response, at["csHash"] + 5, b"\x01"), "the circuit hash differs from the key's")
    _verdict(amd, key, challenge, "the response holds no new contribution")
    _verdict(amd, key, _patch(response, ref.DELTA1, ref.G1_INF_BE), "delta1 or delta2 is the point at infinity")
    _verdict(amd, key, _patch(response, ref.DELTA2, bytes([0x40]) + bytes(127)), "delta1 or delta2 is the point at infinity")


def test_import_old_records_must_begin_the_list(amd, key, response):
    """The key after one contribution (the twin's header and section 10) against responses with two records."""
    h, s10, _ = mref.contribute_ref(key, None, D, S)
    secs = f.read_binfile(key, "zkey", 2)
    order = sorted(secs, key=lambda sid: secs[sid][0][0])
    one = f.write_binfile("zkey", 1, [(sid, {2: h, 10: s10}.get(sid, f.section(key, secs, sid))) for sid in order])
    m = ref.parse_mpcparams(response)
    rec = m["records"][0]
    start = response[:m["at"]["csHash"] + 64]
    other = bytes([rec[320] ^ 1])
    altered = start + struct.pack(">I", 2) + rec[:320] + other + rec[321:] + rec
    _verdict(amd, one, altered, "the contributions do not begin with the key's")
    swapped_in = start + struct.pack(">I", 2) + _patch(rec, 64, rec[128:192]) + rec
    _verdict(amd, one, swapped_in, "the contributions do not begin with the key's")
    _verdict(amd, one, response, "the response holds no new contribution")


def test_import_refuses_a_record_point_off_its_curve(amd, key, response):
    m = ref.parse_mpcparams(response)
    at = m["at"]["records"]
    e = _err(amd, lambda: amd.zkey_import_bellman(key, _patch(response, at + 64 + 32, (5).to_bytes(32, "big")), "x", device=0))
    assert e.code == -2 and str(e) == FORMAT


def test_import_and_export_refuse_a_malformed_key(amd, key, response):
    for call in (lambda z: amd.zkey_export_bellman(z, device=0), lambda z: amd.zkey_import_bellman(z, response, "x", device=0)):
        e = _err(amd, lambda: call(key[:len(key) - 1]))
        assert e.code == -2 and "Invalid File format" in str(e)


def test_no_cpu_path(amd, key, challenge, response):
    if _gpu_present(amd):
        return   # (the GPU suite runs these calls)
    for call in (lambda: amd.zkey_export_bellman(key, device=0), lambda: amd.zkey_bellman_contribute(challenge, D, S, device=0),
                 lambda: amd.zkey_bellman_contribute(challenge, device=0), lambda: amd.zkey_import_bellman(key, response, "x", device=0),
                 lambda: amd.zkey_h_basis(bytes(64 * 4), 2), lambda: amd.zkey_h_basis(bytes(64 * 4), 2, inverse=True)):
        assert _err(amd, call).code == -4
    with pytest.raises(ValueError):
        amd.zkey_h_basis(bytes(64 * 3), 2)
