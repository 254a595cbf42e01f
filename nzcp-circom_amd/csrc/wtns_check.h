// Witness checking (g16_wtns_check): what wtns_check_host.cpp (host: parsing, the CSR builder, the host route, the verdict)
// and wtns_check.hip (the device route) share.
#pragma once
#include "circuit.h"
#include "fr29.cuh"

namespace g16 {

// The three matrices of an R1CS in the layout of QapCsr (internal.h), built once on the host from the .r1cs words:
// per row the +-1 records first (bit 31 of col = minus), then the general ones, whose coefficients are kept as
// coef * 2^522 in the lazy format, so that one product with the PLAIN witness word gives Mont261(coef * w).
struct WcCsr {
  uint32_t m = 0, n_w = 0;
  std::vector<uint32_t> rp[3], mid[3], vptr[3], col[3];   // A, B, C; rp: m + 1, mid and vptr: m
  std::vector<F29> val[3];
  // rows whose longest side -- A, B OR C -- has more than kQapLongRow terms: first the n_mid rows of at most
  // kQapWaveRow terms (eight lanes each), then the rest (a wavefront each)
  std::vector<uint32_t> long_rows;
  uint32_t n_mid = 0, n_long = 0;
};
void wc_build_csr(const Circuit& c, WcCsr& out);

// Device route.  The CSR stays resident; a batch is cut into chunks of `chunk` witnesses, each of which takes
// 72 bytes per wire on the device (the 32-byte plain word and its 40-byte Montgomery image).
struct WcDevice;
int wc_device_create(int device, const WcCsr& csr, uint32_t chunk, WcDevice** out);
// bodies[i] = the n_w canonical words of witness i (host).  first[i] = lowest failing row or 0xffffffff,
// n_failed[i] = the number of failing rows.  ms (optional): upload, kernels (device time, all chunks).
int wc_device_check(WcDevice* d, const uint8_t* const* bodies, size_t count, uint32_t* first, uint32_t* n_failed, float ms[2]);
void wc_device_destroy(WcDevice* d);

}  // namespace g16
