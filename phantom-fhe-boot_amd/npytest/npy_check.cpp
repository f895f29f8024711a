// npy_check — host/npy.cpp on its own: a host-compiler program (no HIP, nothing preloaded) that
// prints what the loader makes of a file, for tests/test_npy_loader.py and for the sanitizer build
// (make SAN=address,undefined builds bin/npy_check_address beside bin/pool_model_address).
//
// usage: npy_check array <file>            shape, then the values in C order
//        npy_check w4 <file>               LoadWeight4D: shape [kH kW in out], values in that order
//        npy_check w2 <file> | w1 <file>   LoadWeight2D / LoadWeight1D
//        npy_check bn <dir> <prefix>       LoadBN: four lines weight, bias, mean, var
//        npy_check image <file> <index>    LoadImage: shape [w w channels], values in that order
// Values are printed as hex doubles (%a), exact.  A refusal prints "refused: <file>: <reason>" and
// exits with status 1; a usage error exits with 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/npy.h"

using namespace phantom;

namespace {

struct PlainBN {
  std::vector<double> weight, bias, mean, var;
};

void print_shape(const std::vector<size_t>& shape) {
  std::printf("shape");
  for (size_t d : shape) std::printf(" %zu", d);
  std::printf("\n");
}

void print_values(const char* label, const std::vector<double>& v) {
  std::printf("%s", label);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  try {
    const std::string what = argc >= 2 ? argv[1] : "";
    if (what == "array" && argc == 3) {
      const NpyArray a = LoadNpy(argv[2]);
      print_shape(a.shape);
      std::printf("item_bytes %zu\n", a.item_bytes);
      print_values("values", a.data);
      return 0;
    }
    if (what == "w4" && argc == 3) {
      const NpyWeight4 w = LoadWeight4D(argv[2]);
      print_shape({w.size(), w[0].size(), w[0][0].size(), w[0][0][0].size()});
      std::vector<double> flat;
      for (const auto& a : w)
        for (const auto& b : a)
          for (const auto& c : b) flat.insert(flat.end(), c.begin(), c.end());
      print_values("values", flat);
      return 0;
    }
    if (what == "w2" && argc == 3) {
      const std::vector<std::vector<double>> w = LoadWeight2D(argv[2]);
      print_shape({w.size(), w[0].size()});
      std::vector<double> flat;
      for (const auto& r : w) flat.insert(flat.end(), r.begin(), r.end());
      print_values("values", flat);
      return 0;
    }
    if (what == "w1" && argc == 3) {
      const std::vector<double> w = LoadWeight1D(argv[2]);
      print_shape({w.size()});
      print_values("values", w);
      return 0;
    }
    if (what == "bn" && argc == 4) {
      const PlainBN bn = LoadBN<PlainBN>(argv[2], argv[3]);
      print_values("weight", bn.weight);
      print_values("bias", bn.bias);
      print_values("mean", bn.mean);
      print_values("var", bn.var);
      return 0;
    }
    if (what == "image" && argc == 4) {
      const NpyTensor3 t = LoadImage(argv[2], std::strtoull(argv[3], nullptr, 10));
      print_shape({t.size(), t[0].size(), t[0][0].size()});
      std::vector<double> flat;
      for (const auto& r : t)
        for (const auto& px : r) flat.insert(flat.end(), px.begin(), px.end());
      print_values("values", flat);
      return 0;
    }
    std::fprintf(stderr, "usage: npy_check array|w4|w2|w1 <file> | bn <dir> <prefix> | image <file> <index>\n");
    return 2;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
    return 1;
  }
}
