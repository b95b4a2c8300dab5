// Stand-alone host program behind tests/test_gru_persist.py: build_gru_persist_images of csrc/weight_images.cpp without a handle, a
// device or HIP.
//
//   gru_persist_dump <blob.bin> <outdir> <enc_depth> <attention> <vocab>
//       what rv_set_option(h, "gru_persistent", 1) builds on the host for a bigru blob of one decoder cell: every image as
//       <outdir>/<name>.bin, one `size <name> <bytes per element> <elements>` line per image and one `scale <name> <hex float>` line
//       per scalar.
#include "weight_images.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
  if (argc != 6) { fprintf(stderr, "usage: gru_persist_dump <blob.bin> <outdir> <enc_depth> <attention> <vocab>\n"); return 2; }
  RvConfig c{};
  c.enc_units = c.dec_units = wimg::U;
  c.enc_depth = atoi(argv[3]); c.dec_depth = 1; c.attention = atoi(argv[4]); c.vocab = atoi(argv[5]);
  const size_t total = wimg::BlobLayout(c, RV_RNN_BIGRU).total;
  std::vector<float> blob(total);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(blob.data(), sizeof(float), total, f) != total || fgetc(f) != EOF) { fprintf(stderr, "%s does not hold the %zu floats of the configuration\n", argv[1], total); return 2; }
  fclose(f);
  const wimg::GruPersistImages im = wimg::build_gru_persist_images(c, blob.data());
  const std::string out = argv[2];
#define X(T, name, count)                                                                          \
  {                                                                                                \
    printf("size %s %zu %zu\n", #name, sizeof(T), im.name.size());                                 \
    FILE* o = fopen((out + "/" #name ".bin").c_str(), "wb");                                       \
    if (!o || fwrite(im.name.data(), sizeof(T), im.name.size(), o) != im.name.size()) { fprintf(stderr, "cannot write %s\n", #name); return 2; } \
    fclose(o);                                                                                     \
  }
  RV_GRU_PERSIST_IMAGES(X)
#undef X
  const wimg::ImageScales& s = im.scales;
  printf("scale kscale %a\nscale uscale %a\nscale cdescale %a\nscale ldescale %a\nscale qdescale %a\n", s.kscale, s.uscale, s.cdescale, s.ldescale, s.qdescale);
  return 0;
}
