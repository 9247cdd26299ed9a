// Stand-alone driver of curdleproofs_amd/csrc/canon_infinity.hpp for tests/test_canon_infinity_cpu.py: the g++ build of the rule that
// Engine::canonical_infinities applies to every input of compressed points under option strict_infinity = 0.
//   stdin:  "ARRAYS", then per array a line "NREC STRIDE NOFF OFF..." and a line with the NREC * STRIDE bytes as hex ("-" for none)
//   stdout: per array, AFTER every array has been processed (each into a store of its own, pre-filled with the bytes "store"), a line
//           "SAME HEX": SAME = 1 if the returned pointer is the input, HEX = what the returned pointer shows; a line "STORE HEX" with the
//           array's store; and "INPUT 1" if the input bytes are what they were
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../curdleproofs_amd/csrc/canon_infinity.hpp"

static void print_hex(const char* tag, const uint8_t* p, size_t n) {
  printf("%s ", tag);
  if (!n) printf("-");
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
  printf("\n");
}

int main() {
  size_t arrays;
  if (!(std::cin >> arrays) || arrays > 16) return 2;
  std::vector<std::vector<uint8_t>> in(arrays), given(arrays), store(arrays);
  std::vector<const uint8_t*> res(arrays);
  for (size_t a = 0; a < arrays; a++) {
    size_t nrec, stride, noff;
    if (!(std::cin >> nrec >> stride >> noff) || nrec > 4096 || stride > 4096 || noff > 8) return 2;
    std::vector<size_t> offs(noff);
    for (size_t& o : offs)
      if (!(std::cin >> o) || o + 48 > stride) return 2;
    std::string h;
    if (!(std::cin >> h)) return 2;
    if (h == "-") h.clear();
    if (h.size() != 2 * nrec * stride) return 2;
    in[a].resize(nrec * stride);   // exactly the bytes: a read behind them is the sanitizer's to report
    for (size_t i = 0; i < in[a].size(); i++) in[a][i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
    given[a] = in[a];
    store[a] = {'s', 't', 'o', 'r', 'e'};
    res[a] = cpx::canonical_infinities(in[a].data(), in[a].size(), nrec, stride, offs, store[a]);
  }
  for (size_t a = 0; a < arrays; a++) {   // every result is read once all calls are behind it
    print_hex(res[a] == in[a].data() ? "1" : "0", res[a], in[a].size());
    print_hex("STORE", store[a].data(), store[a].size());
    printf("INPUT %d\n", in[a] == given[a] ? 1 : 0);
    if (res[a] != in[a].data() && res[a] != store[a].data()) return 3;
  }
  return 0;
}
