// File-path forms of the buffer entry points, for hosts that cannot hold a ceremony file in one buffer (a Node.js
// Buffer ends at 2 GB; powersOfTau28_hez_final_22.ptau is 4.6 GB): the inputs are mapped read-only, the image is written out.
#pragma once
#include <fcntl.h>
#include <stdio.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "binfile.h"

namespace g16 {

struct MappedFile {
  void* p = MAP_FAILED;
  size_t len = 0;
  int open_ro(const char* path) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { set_error(std::string(path) + ": cannot open"); return G16_E_ARG; }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size <= 0) { close(fd); set_error(std::string(path) + ": Invalid File format"); return G16_E_FORMAT; }
    len = (size_t)sb.st_size;
    p = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (p == MAP_FAILED) { set_error(std::string(path) + ": cannot map"); return G16_E_STATE; }
    return G16_OK;
  }
  ~MappedFile() { if (p != MAP_FAILED) munmap(p, len); }
};
// writes z[0, zl) to path in chunks of 256 MB and frees z
inline int write_key_file(const char* path, uint8_t* z, size_t zl) {
  FILE* f = fopen(path, "wb");
  if (!f) { free(z); set_error(std::string(path) + ": cannot create"); return G16_E_ARG; }
  size_t off = 0;
  while (off < zl) {
    const size_t chunk = zl - off < ((size_t)1 << 28) ? zl - off : ((size_t)1 << 28);
    if (fwrite(z + off, 1, chunk, f) != chunk) { fclose(f); free(z); set_error(std::string(path) + ": write failed"); return G16_E_STATE; }
    off += chunk;
  }
  free(z);
  if (fclose(f) != 0) { set_error(std::string(path) + ": write failed"); return G16_E_STATE; }
  return G16_OK;
}

// in_paths[0, nin) mapped in order, call(maps, &image, &len) = the buffer form, its image written to out_path
template <class Call> int files_form(const char* const* in_paths, int nin, const char* out_path, Call call) {
  MappedFile in[2];
  for (int k = 0; k < nin; k++)
    if (const int rc = in[k].open_ro(in_paths[k])) return rc;
  uint8_t* z = nullptr;
  size_t zl = 0;
  if (const int rc = call(in, &z, &zl)) return rc;
  return write_key_file(out_path, z, zl);
}

}  // namespace g16
