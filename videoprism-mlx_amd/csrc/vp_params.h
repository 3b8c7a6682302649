// Error reporting of the C-ABI and the parameter store every handle type is built on: the leaves a
// model expects (name -> shape, in declaration order), their host copies until finalize, and the
// device buffers packed from them.
#pragma once
#include "../../include/videoprism_hip.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace vpi {

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define VP_HIP(expr)                                                                   \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(VP_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

inline uint16_t host_f2bf(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16);  // inf / nan
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

inline std::string shape_str(const int64_t* s, size_t n) {
  std::string r = "(";
  for (size_t i = 0; i < n; ++i) r += std::to_string(s[i]) + (i + 1 < n ? ", " : "");
  return r + ")";
}

struct ParamStore {
  int device = 0;
  bool finalized = false;
  std::vector<std::string> names;  // the expected leaves, in declaration order
  std::map<std::string, std::vector<int64_t>> expected;
  std::map<std::string, std::vector<float>> host;  // leaves set so far; dropped once packed
  std::vector<void*> allocs;                       // device buffers, freed by free_all

  void expect(const std::string& n, std::vector<int64_t> shape) {
    names.push_back(n);
    expected[n] = std::move(shape);
  }

  // the one validation of a leaf handed in through a *_set_param entry point
  int set(const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!name || !data || (ndim > 0 && !shape)) return fail(VP_EINVAL, "null argument");
    if (finalized) return fail(VP_ESTATE, "handle already finalized");
    auto it = expected.find(name);
    if (it == expected.end()) return fail(VP_EINVAL, std::string("unexpected parameter: ") + name);
    const auto& exp = it->second;
    bool ok = (int)exp.size() == ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = exp[i] == shape[i];
    if (!ok)
      return fail(VP_EINVAL, std::string("shape mismatch for ") + name + ": expected " +
                                 shape_str(exp.data(), exp.size()) + " got " + shape_str(shape, ndim < 0 ? 0 : ndim));
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    host[name].assign(data, data + n);
    return VP_OK;
  }

  const std::string* first_missing() const {
    for (const auto& n : names)
      if (!host.count(n)) return &n;
    return nullptr;
  }

  const std::vector<float>& data(const std::string& n) const { return host.at(n); }

  int alloc(size_t bytes, void** out) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return fail(VP_ENOMEM, "hipMalloc failed");
    allocs.push_back(p);
    *out = p;
    return VP_OK;
  }

  int upload(const void* src, size_t bytes, void** out) {
    int rc = alloc(bytes, out);
    if (rc) return rc;
    VP_HIP(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice));
    return VP_OK;
  }

  int upload_f32(const std::vector<float>& v, float** out) {
    void* p = nullptr;
    const int rc = upload(v.data(), v.size() * 4, &p);
    *out = static_cast<float*>(p);
    return rc;
  }

  // matrix in the compute dtype
  int upload_mat(const std::vector<float>& v, bool bf16, void** out) {
    if (!bf16) return upload(v.data(), v.size() * 4, out);
    std::vector<uint16_t> b(v.size());
    for (size_t i = 0; i < v.size(); ++i) b[i] = host_f2bf(v[i]);
    return upload(b.data(), b.size() * 2, out);
  }

  // every leaf packed: the host copies go
  void seal() {
    host.clear();
    finalized = true;
  }

  void free_all() {
    hipSetDevice(device);
    for (void* p : allocs) hipFree(p);
    allocs.clear();
  }
};

}  // namespace vpi
