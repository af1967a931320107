// Packed allow-mask argument of the filtered kNN kernels.
//
// Bit (r & 31) of word (r >> 5) is set when local row r (before row_base)
// may be returned. One mask is shared by every query of a call. Bits at
// positions >= n in the last word are don't-care: no kernel tests them.
#pragma once

#include <torch/extension.h>

// Validates `allow` against the n rows the kernel will score and returns
// its device pointer.
static inline const unsigned int* check_allow_mask(const at::Tensor& allow,
                                                   const at::Tensor& db,
                                                   long long n,
                                                   const char* who) {
  TORCH_CHECK(allow.is_cuda() && allow.scalar_type() == at::kInt &&
                  allow.is_contiguous(),
              who, ": allow must be a contiguous int32 CUDA tensor");
  TORCH_CHECK(allow.device() == db.device(), who,
              ": allow must be on the same device as db");
  TORCH_CHECK(allow.numel() >= (n + 31) / 32, who, ": allow has ",
              allow.numel(), " words, need ", (n + 31) / 32);
  return reinterpret_cast<const unsigned int*>(allow.data_ptr<int>());
}

// Per-row score bias of the bf16 kNN kernels: fp32 [n], indexed like the
// mask by local row (before row_base). The score that enters the top-k is
// dot(q, row) + row_bias[row]. Values must be finite and far above the
// kernels' -1e30 list sentinel; nothing tests for that. Validates
// `row_bias` against the n rows the kernel will score and returns its
// device pointer.
static inline const float* check_row_bias(const at::Tensor& row_bias,
                                          const at::Tensor& db, long long n,
                                          const char* who) {
  TORCH_CHECK(row_bias.is_cuda() && row_bias.scalar_type() == at::kFloat &&
                  row_bias.dim() == 1 && row_bias.is_contiguous(),
              who, ": row_bias must be a contiguous 1D fp32 CUDA tensor");
  TORCH_CHECK(row_bias.device() == db.device(), who,
              ": row_bias must be on the same device as db");
  TORCH_CHECK(row_bias.numel() == n, who, ": row_bias has ", row_bias.numel(),
              " entries, need ", n);
  return row_bias.data_ptr<float>();
}
