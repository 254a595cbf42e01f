// The .ptau reader of the routes that take a ceremony file (PLONK setup, Groth16 setup, prepare phase2, and the ptau leg
// of zkey verify, which opens with ptau_open and reads section 2 alone).
#pragma once
#include <functional>

#include "binfile.h"

namespace g16 {

struct PtauView : BinView {
  uint32_t power = 0;
  int blocks[16] = {};   // sections 12-15: whole blocks present
};

int ptau_bad(const char* why);   // sets "ptau: <why>" -> G16_E_FORMAT

// Container, bn128 section 1 and the power: shared by the PLONK route, the prepared reader and g16_ptau_prepare.
// tau_sections: sections 2 and 3 must be there too, their absence reported with the curve text ahead of the power
// check.  That is the PLONK route's order, and it cannot check them itself after this call: a file without section 2
// AND with a power above 28 would then get the bare text of the power check instead of the curve text.  The other two
// routes check the sections they read after the power, with the bare text, and pass false.
int ptau_open(const uint8_t* ptau, size_t ptau_len, PtauView& v, bool tau_sections);
// ptau_open and the prepared-section block layout (sections 12-15, v.blocks)
int ptau_open_prepared(const uint8_t* ptau, size_t ptau_len, PtauView& v);

// g16_groth16_setup_ptau (setup_groth16.cpp) with a caller's check of the opened ptau for the key's domain 2^log_n, run
// after the setup's own checks and before the device is asked for (`zkey new` with the circuit hash reads section 2 too)
using SetupPtauCheck = std::function<int(const PtauView& pv, int log_n)>;
int groth16_setup_ptau_checked(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                               uint8_t** zkey, size_t* zkey_len, const SetupPtauCheck* before_device);

}  // namespace g16
