// The circuit hash (csHash) that `zkey new` stores at the head of section 10 (zkey_cshash_host.cpp, zkey_cshash.hip).
// Host code.
#pragma once
#include "ptau.h"
#include "zkey_mpc.h"

namespace g16 {

// What the hash reads of a ceremony file for a key of domain 2^log_n, checked on the host with the texts of
// g16_zkey_verify_from_init_ptau: section 2 holds at least 2N - 1 points, every one with coordinates below q and on the
// curve, else G16_E_FORMAT "ptau: Invalid File format".  (The power is the caller's question: its text differs by entry.)
int cshash_check_ptau(const PtauView& pv, int log_n);
// csHash of the INITIAL key k (gamma = delta = 1, no records; not checked here) over the ceremony's section 2, on
// `device`; the inputs have passed open_key and cshash_check_ptau.  Section 9 and the bytes in section 10 are not read.
int zkey_cs_hash_core(const KeyView& k, const PtauView& pv, int device, uint8_t out[64]);

}  // namespace g16
