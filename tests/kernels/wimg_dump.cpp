// Stand-alone host program behind tests/test_weight_images.py: csrc/weight_images.cpp without a handle, a device or HIP.
//
//   wimg_dump images <blob.bin> <outdir> <rnn 0|1> <enc_depth> <dec_depth> <attention> <vocab> <weight_parts>
//       what rv_load_weights does on the host: rounds the blob where weight_parts is 1, builds every image and writes each one built
//       as <outdir>/<name>.bin.  Prints `total <floats of the blob>`, one `size <name> <bytes per element> <elements>` line per image a
//       handle of that configuration allocates, and one `scale <name> <hex float>` line per scalar.
//   wimg_dump round <blob.bin> <out.bin> <enc_depth> <dec_depth> <vocab>
//       round_blob_weights alone.
//   wimg_dump pack <recurrent3|recurrent4|wh|wq16> <in.bin> <out.bin>
//       one image family's packer on every matrix of in.bin (back to back), the images back to back in out.bin; wq16 prints its scales.
#include "weight_images.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace {

std::vector<float> read_floats(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<float> v((size_t)n / sizeof(float));
  if (fread(v.data(), sizeof(float), v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
  fclose(f);
  return v;
}

void write_bytes(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

RvConfig config(int enc_depth, int dec_depth, int attention, int vocab) {
  RvConfig c{};
  c.enc_units = c.dec_units = wimg::U;
  c.enc_depth = enc_depth; c.dec_depth = dec_depth; c.attention = attention; c.vocab = vocab;
  return c;
}

int images(char** a) {
  std::vector<float> blob = read_floats(a[0]);
  const std::string out = a[1];
  const int rnn = atoi(a[2]), parts = atoi(a[7]);
  const RvConfig c = config(atoi(a[3]), atoi(a[4]), atoi(a[5]), atoi(a[6]));
  const wimg::BlobLayout lay(c, rnn);
  printf("total %zu\n", lay.total);
  if (blob.size() != lay.total) { fprintf(stderr, "blob has %zu floats, the configuration needs %zu\n", blob.size(), lay.total); return 2; }
  if (parts == 1) wimg::round_blob_weights(c, blob.data());
  const wimg::ImageCounts cnt = wimg::image_counts(c, rnn);
  const wimg::HostImages im = wimg::build_weight_images(c, rnn, parts, blob.data());
#define X(T, name, count)                                                                         \
  if (cnt.name) printf("size %s %zu %zu\n", #name, sizeof(T), cnt.name);                          \
  if (!im.name.empty()) write_bytes(out + "/" #name ".bin", im.name.data(), im.name.size() * sizeof(T));
  RV_WEIGHT_IMAGES(X)
#undef X
  const wimg::ImageScales& s = im.scales;
  printf("scale kscale %a\nscale uscale %a\nscale cdescale %a\nscale ldescale %a\nscale qdescale %a\nscale c1descale %a\n",
         s.kscale, s.uscale, s.cdescale, s.ldescale, s.qdescale, s.c1descale);
  return 0;
}

int round_only(char** a) {
  std::vector<float> blob = read_floats(a[0]);
  const RvConfig c = config(atoi(a[2]), atoi(a[3]), 0, atoi(a[4]));
  if (blob.size() != wimg::BlobLayout(c, RV_RNN_BILSTM).total) { fprintf(stderr, "blob size\n"); return 2; }
  wimg::round_blob_weights(c, blob.data());
  write_bytes(a[1], blob.data(), blob.size() * sizeof(float));
  return 0;
}

int pack(char** a) {
  const std::string kind = a[0];
  const std::vector<float> in = read_floats(a[1]);
  const int g = kind == "recurrent3" ? 3 : 4;
  size_t rows_cols, slot;
  if (kind == "recurrent3" || kind == "recurrent4") { rows_cols = (size_t)wimg::U * g * wimg::U; slot = wimg::ua_slot(g); }
  else if (kind == "wh") { rows_cols = (size_t)wimg::E * 4 * wimg::U; slot = wimg::WH_SLOT; }
  else if (kind == "wq16") { rows_cols = (size_t)wimg::U * wimg::U; slot = (size_t)2 * wimg::U * wimg::U; }
  else { fprintf(stderr, "unknown image family %s\n", a[0]); return 2; }
  if (in.empty() || in.size() % rows_cols) { fprintf(stderr, "%s: %zu floats are no whole matrices of %zu\n", a[1], in.size(), rows_cols); return 2; }
  const size_t n = in.size() / rows_cols;
  std::vector<uint16_t> img(n * slot, 0);
  for (size_t i = 0; i < n; ++i) {
    const float* m = in.data() + i * rows_cols;
    uint16_t* o = img.data() + i * slot;
    if (kind == "wh") wimg::pack_wh(m, o);
    else if (kind == "wq16") printf("scale %a\n", wimg::pack_wq16(m, o));
    else wimg::pack_recurrent(m, g, o);
  }
  write_bytes(a[2], img.data(), img.size() * sizeof(uint16_t));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 10 && !strcmp(argv[1], "images")) return images(argv + 2);
  if (argc == 7 && !strcmp(argv[1], "round")) return round_only(argv + 2);
  if (argc == 5 && !strcmp(argv[1], "pack")) return pack(argv + 2);
  fprintf(stderr, "usage: wimg_dump images|round|pack ... (see the head of tests/kernels/wimg_dump.cpp)\n");
  return 2;
}
