// npy.h — a reader for NumPy's .npy array files, written from the format description (NEP 1,
// numpy/lib/format.py's docstring), and the weight-file helpers of the reference's Resnet/ program
// (LoadWeight4D / 2D / 1D, LoadBN, LoadImage) on top of it.  Host code only: no HIP include, so a
// host compiler builds it alone (npytest/npy_check.cpp).
//
// A file is: the magic "\x93NUMPY", a major and a minor version byte, a little-endian header length
// (2 bytes in version 1.0, 4 in 2.0), that many bytes of an ASCII Python dict literal with the keys
// 'descr', 'fortran_order' and 'shape', then the array's bytes.
//
// Accepted: versions 1.0 and 2.0; descr '<f4' or '<f8' (little-endian IEEE floats); fortran_order
// False; 1 to 4 dimensions, none of them 0, whose product times the item size is exactly the number
// of bytes after the header.  Everything else is refused with a std::runtime_error naming the file
// and the reason; no byte outside the file's contents is ever read.
#pragma once

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace phantom {

struct BNParams;  // host/dnn.h: weight, bias, mean, var
using NpyWeight4 = std::vector<std::vector<std::vector<std::vector<double>>>>;  // DNN::Weight4
using NpyTensor3 = std::vector<std::vector<std::vector<double>>>;               // DNN::Tensor3

struct NpyArray {
  std::vector<size_t> shape;
  std::vector<double> data;  // C order; an f4 file's values widened exactly
  size_t item_bytes = 0;     // 4 or 8, as stored
};

// parse a whole file's contents (`name` is only used in error messages)
NpyArray ParseNpy(const unsigned char* bytes, size_t size, const std::string& name);
NpyArray LoadNpy(const std::string& path);

// PyTorch's (out, in, kH, kW) file -> DNN::Weight4 [kH][kW][in][out]
NpyWeight4 LoadWeight4D(const std::string& path);
// (rows, cols) -> [rows][cols] (a fully connected layer's (classes, features))
std::vector<std::vector<double>> LoadWeight2D(const std::string& path);
std::vector<double> LoadWeight1D(const std::string& path);
// <dir>/<prefix>_weight.npy, _bias, _running_mean, _running_var: four 1-D files of one length
// (a template only so that this header needs no dnn.h: LoadBN(dir, prefix) returns BNParams)
template <class BN = BNParams>
BN LoadBN(const std::string& dir, const std::string& prefix) {
  BN bn;
  bn.weight = LoadWeight1D(dir + "/" + prefix + "_weight.npy");
  bn.bias = LoadWeight1D(dir + "/" + prefix + "_bias.npy");
  bn.mean = LoadWeight1D(dir + "/" + prefix + "_running_mean.npy");
  bn.var = LoadWeight1D(dir + "/" + prefix + "_running_var.npy");
  if (bn.bias.size() != bn.weight.size() || bn.mean.size() != bn.weight.size() || bn.var.size() != bn.weight.size())
    throw std::runtime_error(dir + "/" + prefix + "_*.npy: the four batch-norm files differ in length");
  return bn;
}
// image `index` of an (images, channels, w, w) file -> DNN::Tensor3 [w][w][channel]
NpyTensor3 LoadImage(const std::string& path, size_t index);

}  // namespace phantom
