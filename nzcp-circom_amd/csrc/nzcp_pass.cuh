// The front end of NZ COVID Pass verification for host and device: pass URI text -> base32 -> COSE_Sign1 / CWT walk ->
// SHA-256(ToBeSigned), SHA-256("given,family,dob"), nbf / exp, the issuer-key index and the signature's place.  The
// contract is the one written in include/g16_prover.h ("NZCP pass verification from URIs"); js/nzcpInput.js and
// js/index.js::verifyPass are the one-pass-at-a-time twin.
//
// Passes are attacker-supplied bytes: every read of the decoded bytes goes through pass_at, which takes the buffer
// length; every length is compared with what is left before it is used; the skip of an arbitrary item is iterative on a
// stack of kPassCborDepth counters that the caller supplies (LDS on the device, so nothing is indexed through scratch).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/g16_prover.h"
#include "sha256.cuh"

namespace g16 {

constexpr uint32_t kPassUriMax = G16_PASS_URI_MAX;                 // bytes of URI text per pass
constexpr uint32_t kPassCborDepth = G16_PASS_CBOR_DEPTH;           // containers open at once inside a skipped item
constexpr uint32_t kPassDecodedMax = (kPassUriMax * 5) / 8;        // 1280: decoded bytes of kPassUriMax characters
constexpr uint32_t kPassNameMax = G16_PASS_NAME_MAX;               // bytes of a key's iss, and of its kid
constexpr uint32_t kPassB32Stride = 4 + kPassDecodedMax;           // op 0: u32 length, then the bytes
constexpr uint32_t kPassB32Invalid = 0xffffffffu;                  // op 0: the length of an item that is not base32

// the issuer keys' names, resident next to the ES256 tables: key j is found by iss and kid, bytewise
struct PassKeyName {
  uint32_t iss_len, kid_len;
  uint8_t iss[kPassNameMax], kid[kPassNameMax];
};

// ---------------------------------------------------------------- the decoded bytes
struct PassBuf {
  const uint8_t* p;
  uint32_t len;
};
// THE accessor: byte i of the decoded pass, 0 past its end (callers have compared with len before; this is the net)
G16_HD uint32_t pass_at(const PassBuf& b, uint32_t i) { return i < b.len ? b.p[i] : 0u; }

// ---------------------------------------------------------------- text and base32
G16_HD bool pass_is_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
G16_HD int pass_b32_value(uint8_t c) {   // RFC 4648 alphabet, upper case only
  return c >= 'A' && c <= 'Z' ? c - 'A' : c >= '2' && c <= '7' ? c - '2' + 26 : -1;
}
// text[0, n) without its trailing '=': the count of characters left
G16_HD uint32_t pass_b32_body(const uint8_t* text, uint32_t n) {
  while (n > 0 && text[n - 1] == '=') n--;
  return n;
}
// Rule 1 on text[0, n), n <= kPassUriMax: trimmed, "NZCP:/1/", at least one base32 character, then only '='.
// -> where the base32 characters start and how many they are (their alphabet is checked by the decoder)
G16_HD bool pass_text_frame(const uint8_t* text, uint32_t n, uint32_t* start, uint32_t* n_chars) {
  uint32_t lo = 0;
  while (lo < n && pass_is_space(text[lo])) lo++;
  while (n > lo && pass_is_space(text[n - 1])) n--;
  if (n - lo < 8) return false;
  const uint64_t want = 0x4e5a43503a2f312full;   // "NZCP:/1/"
  uint64_t got = 0;
  for (uint32_t k = 0; k < 8; k++) got = got << 8 | text[lo + k];
  if (got != want) return false;
  lo += 8;
  const uint32_t body = pass_b32_body(text + lo, n - lo);
  if (body == 0) return false;
  *start = lo;
  *n_chars = body;
  return true;
}
G16_HD uint32_t pass_b32_bytes(uint32_t n_chars) { return (uint32_t)(((uint64_t)n_chars * 5) / 8); }
// Group g of the base32 characters chars[0, n_chars): 8 characters -> 5 bytes at out[5 g ...], those below n_out.  The
// last group may be short: its characters fill the top of the 40 bits, the leftover bits are dropped without a check.
// false: a character outside the alphabet.  Groups are independent: lanes stride over them.
G16_HD bool pass_b32_group(const uint8_t* chars, uint32_t n_chars, uint32_t g, uint8_t* out, uint32_t n_out) {
  uint64_t acc = 0;
  bool good = true;
  for (uint32_t k = 0; k < 8; k++) {
    const uint32_t i = 8 * g + k;
    int v = 0;
    if (i < n_chars) {
      v = pass_b32_value(chars[i]);
      if (v < 0) { good = false; v = 0; }
    }
    acc = acc << 5 | (uint64_t)v;
  }
  for (uint32_t k = 0; k < 5; k++) {
    const uint32_t o = 5 * g + k;
    if (o < n_out) out[o] = (uint8_t)(acc >> (8 * (4 - k)));
  }
  return good;
}
// all groups, one after the other (the host route, and the layer operator's op 0)
G16_HD bool pass_b32_decode(const uint8_t* chars, uint32_t n_chars, uint8_t* out, uint32_t n_out) {
  bool good = true;
  for (uint32_t g = 0; g < (n_chars + 7) / 8; g++) good = pass_b32_group(chars, n_chars, g, out, n_out) && good;
  return good;
}

// ---------------------------------------------------------------- CBOR
// The head at pos inside [pos, end): major type 0..6, additional info < 24 or 24..27 (non-minimal accepted); 28..31 and
// major type 7 are refused.  body = the position after the head.
G16_HD bool cbor_head(const PassBuf& b, uint32_t end, uint32_t pos, uint32_t* major, uint64_t* arg, uint32_t* body) {
  if (end > b.len || pos >= end) return false;
  const uint32_t head = pass_at(b, pos), info = head & 31u;
  *major = head >> 5;
  if (*major == 7 || info > 27) return false;
  pos++;
  uint64_t a = info;
  if (info >= 24) {
    const uint32_t n = 1u << (info - 24);
    if (n > end - pos) return false;
    a = 0;
    for (uint32_t k = 0; k < n; k++) a = a << 8 | pass_at(b, pos + k);
    pos += n;
  }
  *arg = a;
  *body = pos;
  return true;
}
// a byte or text string's head at pos, its bytes inside [.., end): off / len of the bytes, next = after them
G16_HD bool cbor_string(const PassBuf& b, uint32_t end, uint32_t pos, uint32_t* major, uint32_t* off, uint32_t* len, uint32_t* next) {
  uint64_t a;
  uint32_t body;
  if (!cbor_head(b, end, pos, major, &a, &body) || (*major != 2 && *major != 3) || a > end - body) return false;
  *off = body;
  *len = (uint32_t)a;
  *next = body + (uint32_t)a;
  return true;
}
// Validate and skip ONE item at *pos inside [*pos, end), iteratively: stack[0, kPassCborDepth) holds the items still to
// come of every open array (n), map (2 n) and tag (1); an empty array or map opens nothing.  A count above the bytes
// left cannot be met (an item is at least a byte), so it is refused before it is stored.
G16_HD bool cbor_skip(const PassBuf& b, uint32_t end, uint32_t* pos, uint32_t* stack) {
  uint32_t sp = 0, p = *pos;
  for (;;) {
    uint32_t major, body;
    uint64_t a;
    if (!cbor_head(b, end, p, &major, &a, &body)) return false;
    p = body;
    uint32_t open = 0;
    if (major == 2 || major == 3) {
      if (a > end - p) return false;
      p += (uint32_t)a;
    } else if (major == 4 || major == 5) {
      if (a > (end - p) >> (major - 4)) return false;
      open = (uint32_t)a << (major - 4);
    } else if (major == 6) {
      open = 1;
    }
    if (open) {
      if (sp == kPassCborDepth) return false;
      stack[sp++] = open;
      continue;
    }
    while (sp > 0 && --stack[sp - 1] == 0) sp--;   // the item ends every container it was the last of
    if (sp == 0) break;
  }
  *pos = p;
  return true;
}
// a map's head at pos: the number of pairs (each at least two bytes), body = the first key
G16_HD bool cbor_map(const PassBuf& b, uint32_t end, uint32_t pos, uint32_t* pairs, uint32_t* body) {
  uint32_t major;
  uint64_t a;
  if (!cbor_head(b, end, pos, &major, &a, body) || major != 5 || a > (end - *body) >> 1) return false;
  *pairs = (uint32_t)a;
  return true;
}
// is the item at pos the text string name[0, n)?
G16_HD bool cbor_is_text(const PassBuf& b, uint32_t end, uint32_t pos, const char* name, uint32_t n) {
  uint32_t major, off, len, next;
  if (!cbor_string(b, end, pos, &major, &off, &len, &next) || major != 3 || len != n) return false;
  bool same = true;
  for (uint32_t k = 0; k < n; k++) same = same && pass_at(b, off + k) == (uint8_t)name[k];
  return same;
}
// the value of the item at pos when it is an unsigned integer (any width), else ~0
G16_HD uint64_t cbor_uint_or_none(const PassBuf& b, uint32_t end, uint32_t pos) {
  uint32_t major, body;
  uint64_t a;
  return cbor_head(b, end, pos, &major, &a, &body) && major == 0 ? a : ~0ull;
}
G16_HD bool cbor_is_map(const PassBuf& b, uint32_t end, uint32_t pos) {
  uint32_t major, body;
  uint64_t a;
  return cbor_head(b, end, pos, &major, &a, &body) && major == 5;
}

// ---------------------------------------------------------------- what the walk finds
// state of a claim: 0 absent, 1 present and of the wanted type, 2 present and of another type.  A later duplicate of a
// key overrides an earlier one, as a Map filled in order does.
struct PassText {
  uint32_t off, len, state;
};
struct PassInt {   // state 2 also for an integer outside int64
  int64_t v;
  uint32_t state;
};
struct PassParsed {
  uint32_t prot_off, prot_len, payload_off, payload_len, sig_off;
  uint32_t alg_state;   // 1: the integer -7
  PassText kid, iss, given, family, dob;
  PassInt nbf, exp;
  uint32_t subj_state;   // 1: "vc" is a map whose "credentialSubject" is a map
};

G16_HD void pass_take_text(const PassBuf& b, uint32_t end, uint32_t pos, bool bytes_too, PassText* t) {
  uint32_t major, next;
  t->state = 2;
  if (cbor_string(b, end, pos, &major, &t->off, &t->len, &next) && (major == 3 || bytes_too)) t->state = 1;
}
G16_HD void pass_take_int(const PassBuf& b, uint32_t end, uint32_t pos, PassInt* t) {
  uint32_t major, body;
  uint64_t a;
  t->state = 2;
  if (!cbor_head(b, end, pos, &major, &a, &body) || major > 1 || a > 0x7fffffffffffffffull) return;
  t->v = major == 0 ? (int64_t)a : -1 - (int64_t)a;
  t->state = 1;
}

// "credentialSubject": a map at *pos
G16_HD bool pass_scan_subject(const PassBuf& b, uint32_t end, uint32_t* pos, uint32_t* stack, PassParsed* out) {
  uint32_t pairs, p;
  if (!cbor_map(b, end, *pos, &pairs, &p)) return false;
  out->given.state = out->family.state = out->dob.state = 0;
  for (uint32_t i = 0; i < pairs; i++) {
    const uint32_t key = p;
    if (!cbor_skip(b, end, &p, stack)) return false;
    if (cbor_is_text(b, end, key, "givenName", 9)) pass_take_text(b, end, p, false, &out->given);
    else if (cbor_is_text(b, end, key, "familyName", 10)) pass_take_text(b, end, p, false, &out->family);
    else if (cbor_is_text(b, end, key, "dob", 3)) pass_take_text(b, end, p, false, &out->dob);
    if (!cbor_skip(b, end, &p, stack)) return false;
  }
  *pos = p;
  return true;
}
// "vc": a map at *pos; its last "credentialSubject" decides
G16_HD bool pass_scan_vc(const PassBuf& b, uint32_t end, uint32_t* pos, uint32_t* stack, PassParsed* out) {
  uint32_t pairs, p;
  if (!cbor_map(b, end, *pos, &pairs, &p)) return false;
  out->subj_state = 0;
  for (uint32_t i = 0; i < pairs; i++) {
    const uint32_t key = p;
    if (!cbor_skip(b, end, &p, stack)) return false;
    if (cbor_is_text(b, end, key, "credentialSubject", 17)) {
      out->subj_state = 2;
      if (cbor_is_map(b, end, p)) {
        if (!pass_scan_subject(b, end, &p, stack, out)) return false;
        out->subj_state = 1;
        continue;
      }
    }
    if (!cbor_skip(b, end, &p, stack)) return false;
  }
  *pos = p;
  return true;
}
// the CWT claims: the first item of the payload's bytes must be a map
G16_HD bool pass_scan_payload(const PassBuf& b, PassParsed* out, uint32_t* stack) {
  const uint32_t end = out->payload_off + out->payload_len;
  uint32_t pairs, p;
  if (!cbor_map(b, end, out->payload_off, &pairs, &p)) return false;
  out->iss.state = out->nbf.state = out->exp.state = out->subj_state = 0;
  out->given.state = out->family.state = out->dob.state = 0;
  for (uint32_t i = 0; i < pairs; i++) {
    const uint32_t key = p;
    if (!cbor_skip(b, end, &p, stack)) return false;
    const uint64_t k = cbor_uint_or_none(b, end, key);
    if (k == 1) pass_take_text(b, end, p, false, &out->iss);
    else if (k == 4) pass_take_int(b, end, p, &out->exp);
    else if (k == 5) pass_take_int(b, end, p, &out->nbf);
    else if (cbor_is_text(b, end, key, "vc", 2)) {
      out->subj_state = 2;
      if (cbor_is_map(b, end, p)) {
        if (!pass_scan_vc(b, end, &p, stack, out)) return false;
        continue;
      }
    }
    if (!cbor_skip(b, end, &p, stack)) return false;
  }
  return out->iss.state == 1 && out->nbf.state == 1 && out->exp.state == 1 && out->subj_state == 1;
}
// the protected header: the first item of its bytes must be a map; key 1 alg, key 4 kid
G16_HD bool pass_scan_protected(const PassBuf& b, PassParsed* out, uint32_t* stack) {
  const uint32_t end = out->prot_off + out->prot_len;
  uint32_t pairs, p;
  if (!cbor_map(b, end, out->prot_off, &pairs, &p)) return false;
  out->alg_state = 0;
  out->kid.state = 0;
  for (uint32_t i = 0; i < pairs; i++) {
    const uint32_t key = p;
    if (!cbor_skip(b, end, &p, stack)) return false;
    const uint64_t k = cbor_uint_or_none(b, end, key);
    if (k == 1) {
      uint32_t major, body;
      uint64_t a;
      out->alg_state = cbor_head(b, end, p, &major, &a, &body) && major == 1 && a == 6 ? 1 : 2;
    } else if (k == 4) {
      pass_take_text(b, end, p, true, &out->kid);
    }
    if (!cbor_skip(b, end, &p, stack)) return false;
  }
  return true;
}
// COSE_Sign1: tag 18 around an array of exactly 4: bstr, any item, bstr, bstr of 64 bytes; what follows is ignored
G16_HD bool pass_scan_cose(const PassBuf& b, PassParsed* out, uint32_t* stack) {
  uint32_t major, body, p, next, sig_len;
  uint64_t a;
  if (!cbor_head(b, b.len, 0, &major, &a, &body) || major != 6 || a != 18) return false;
  if (!cbor_head(b, b.len, body, &major, &a, &p) || major != 4 || a != 4) return false;
  if (!cbor_string(b, b.len, p, &major, &out->prot_off, &out->prot_len, &next) || major != 2) return false;
  p = next;
  if (!cbor_skip(b, b.len, &p, stack)) return false;
  if (!cbor_string(b, b.len, p, &major, &out->payload_off, &out->payload_len, &next) || major != 2) return false;
  if (!cbor_string(b, b.len, next, &major, &out->sig_off, &sig_len, &next) || major != 2) return false;
  return sig_len == 64;
}

// ---------------------------------------------------------------- the two digests, streamed from where the bytes lie
// bytes of a byte string's head as nzcpInput.js::bstrHeader writes them (len < 65536 here: a pass is at most 1280 bytes)
G16_HD uint32_t pass_bstr_head_len(uint32_t len) { return len < 24 ? 1 : len < 256 ? 2 : 3; }
G16_HD uint32_t pass_bstr_head_byte(uint32_t len, uint32_t k) {
  if (len < 24) return 0x40 + len;
  if (len < 256) return k == 0 ? 0x58 : len;
  return k == 0 ? 0x59 : k == 1 ? len >> 8 : len & 0xff;
}
// ToBeSigned = 84 6A "Signature1" bstr(protected) 40 bstr(payload)
struct PassTbsSource {
  PassBuf b;
  uint32_t prot_off, prot_len, payload_off, payload_len;
  G16_HD uint32_t length() const {
    return 12 + pass_bstr_head_len(prot_len) + prot_len + 1 + pass_bstr_head_len(payload_len) + payload_len;
  }
  G16_HD uint32_t operator()(uint32_t pos) const {
    if (pos < 12) {   // 84 6A 53 69 67 6E 61 74 75 72 65 31
      const uint64_t hi = 0x846a5369676e6174ull, lo = 0x75726531ull;
      return (uint32_t)(pos < 8 ? hi >> (8 * (7 - pos)) : lo >> (8 * (11 - pos))) & 0xffu;
    }
    pos -= 12;
    const uint32_t h1 = pass_bstr_head_len(prot_len);
    if (pos < h1) return pass_bstr_head_byte(prot_len, pos) & 0xffu;
    pos -= h1;
    if (pos < prot_len) return pass_at(b, prot_off + pos);
    pos -= prot_len;
    if (pos == 0) return 0x40u;
    pos -= 1;
    const uint32_t h2 = pass_bstr_head_len(payload_len);
    if (pos < h2) return pass_bstr_head_byte(payload_len, pos) & 0xffu;
    pos -= h2;
    return pass_at(b, payload_off + pos);
  }
};
// given "," family "," dob
struct PassSubjectSource {
  PassBuf b;
  PassText given, family, dob;
  G16_HD uint32_t length() const { return given.len + family.len + dob.len + 2; }
  G16_HD uint32_t operator()(uint32_t pos) const {
    if (pos < given.len) return pass_at(b, given.off + pos);
    pos -= given.len;
    if (pos == 0) return ',';
    pos -= 1;
    if (pos < family.len) return pass_at(b, family.off + pos);
    pos -= family.len;
    if (pos == 0) return ',';
    return pass_at(b, dob.off + pos - 1);
  }
};
// plain bytes (the layer operator's op 1)
struct PassBytesSource {
  const uint8_t* p;
  G16_HD uint32_t operator()(uint32_t pos) const { return p[pos]; }
};

// ---------------------------------------------------------------- the key by its name
G16_HD bool pass_name_equals(const PassBuf& b, const PassText& t, const uint8_t* name, uint32_t n) {
  if (t.len != n) return false;
  bool same = true;
  for (uint32_t k = 0; k < n; k++) same = same && pass_at(b, t.off + k) == name[k];
  return same;
}
// the first key whose iss and kid equal the pass's, or n_keys
G16_HD uint32_t pass_find_key(const PassBuf& b, const PassParsed& ps, const PassKeyName* keys, uint32_t n_keys) {
  if (ps.kid.state != 1) return n_keys;
  for (uint32_t j = 0; j < n_keys; j++)
    if (pass_name_equals(b, ps.iss, keys[j].iss, keys[j].iss_len) && pass_name_equals(b, ps.kid, keys[j].kid, keys[j].kid_len)) return j;
  return n_keys;
}

// ---------------------------------------------------------------- the front end of one pass
G16_HD void pass_result_clear(g16_pass_result* r, uint32_t verdict) {
  r->verdict = verdict;
  r->key_idx = r->tbs_len = r->flags = 0;
  r->nbf = r->exp = 0;
  for (int k = 0; k < 32; k++) r->tbs_sha256[k] = r->cred_subj_sha256[k] = 0;
}
// Rules 3 to 6 on the decoded bytes: the record with verdict 0 (nothing against the pass before its signature), 1, 2 or
// 3; *sig_off = where the 64 signature bytes lie when the verdict is 0.  A well-formed pass has every field filled
// whatever its verdict (key_idx = 0 when no key matched); a malformed one has none.
G16_HD void pass_front(const PassBuf& b, const PassKeyName* keys, uint32_t n_keys, uint32_t* stack, g16_pass_result* r,
                       uint32_t* sig_off) {
  PassParsed ps;
  pass_result_clear(r, G16_PASS_MALFORMED);
  *sig_off = 0;
  if (!pass_scan_cose(b, &ps, stack) || !pass_scan_protected(b, &ps, stack) || !pass_scan_payload(b, &ps, stack)) return;
  const uint32_t key = pass_find_key(b, ps, keys, n_keys);
  r->verdict = ps.alg_state != 1 ? G16_PASS_ALG : key == n_keys ? G16_PASS_KEY : G16_PASS_OK;
  r->key_idx = key == n_keys ? 0 : key;
  r->nbf = ps.nbf.v;
  r->exp = ps.exp.v;
  const PassTbsSource tbs{b, ps.prot_off, ps.prot_len, ps.payload_off, ps.payload_len};
  r->tbs_len = tbs.length();
  sha256_stream(tbs, r->tbs_len, r->tbs_sha256);
  if (ps.given.state == 1 && ps.family.state == 1 && ps.dob.state == 1) {
    const PassSubjectSource subj{b, ps.given, ps.family, ps.dob};
    r->flags |= G16_PASS_HAS_SUBJECT;
    sha256_stream(subj, subj.length(), r->cred_subj_sha256);
  }
  *sig_off = ps.sig_off;
}

// ---------------------------------------------------------------- the holder's side: the circuit's input words
// NZCPPubIdentity's inputs are toBeSigned (8 M words, a bit each, MSB first per byte, zero beyond the length) and
// toBeSignedLen: 8 M + 1 words of 32 bytes in standard form, the image g16_nzcp_inputs writes.  M is at most its bound.
constexpr uint32_t kPassInputsMaxBytes = 503;
G16_HD uint32_t pass_input_count(uint32_t max_bytes) { return 8 * max_bytes + 1; }
// where ToBeSigned's two byte strings lie: the COSE_Sign1 walk alone, nothing of the claims is read
G16_HD bool pass_tbs_locate(const PassBuf& b, uint32_t* stack, PassTbsSource* tbs) {
  PassParsed ps;
  if (!pass_scan_cose(b, &ps, stack)) return false;
  *tbs = PassTbsSource{b, ps.prot_off, ps.prot_len, ps.payload_off, ps.payload_len};
  return true;
}
// the low 32 bits of input word k < 8 M + 1 (the other 28 bytes of a word are zero); tbs_len <= max_bytes
G16_HD uint32_t pass_input_word(const PassTbsSource& tbs, uint32_t tbs_len, uint32_t max_bytes, uint32_t k) {
  if (k >= 8 * max_bytes) return tbs_len;
  const uint32_t at = k >> 3;
  return at < tbs_len ? (tbs(at) >> (7 - (k & 7))) & 1u : 0u;
}

// the relying party's last step: the signature's verdict, then nbf / exp against `now`
G16_HD uint32_t pass_merge(uint32_t verdict, bool sig_ok, int64_t nbf, int64_t exp, int64_t now) {
  if (verdict != G16_PASS_OK) return verdict;
  return !sig_ok ? G16_PASS_SIGNATURE : now < nbf ? G16_PASS_NOT_YET : now >= exp ? G16_PASS_EXPIRED : G16_PASS_OK;
}

}  // namespace g16
