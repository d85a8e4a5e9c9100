// Context helpers every translation unit calls (declared in ctx.h): error text, device buffers and their accounting, copies
// in and out, the upload helper, the phase stopwatch, the Schur column-block width, and the drops of a block's buffer subsets.
#include <cstdarg>
#include <algorithm>

#include "ctx.h"

namespace lrn {

int set_error(lrn_ctx* c, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  (void)hipGetLastError();
  return code;
}

int ensure(lrn_ctx* c, DBuf& b, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 8;
  if (b.bytes < bytes) {
    if (b.p) (void)hipFree(b.p);
    if (b.acct) *b.acct -= b.bytes;
    b.p = nullptr;
    b.bytes = 0;
    b.acct = nullptr;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess)
      return set_error(c, LRN_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    b.bytes = bytes;
    if (c) {
      b.acct = &c->dev_bytes;
      c->dev_bytes += bytes;
      c->dev_bytes_peak = std::max(c->dev_bytes_peak, c->dev_bytes);
    }
    zero = true;
  }
  if (zero) LRN_HIP(c, hipMemsetAsync(b.p, 0, b.bytes, c->stream));
  return LRN_OK;
}

void release(DBuf& b) {
  if (b.p) (void)hipFree(b.p);
  if (b.p && b.acct) *b.acct -= b.bytes;
  b.p = nullptr;
  b.bytes = 0;
  b.acct = nullptr;
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// Column-block width of the Schur sharding.  Auto: two blocks per rank (the snake map pairs a long early
// block with a short late one, so two are enough to balance the triangle), rounded up to the 128-column
// tile: the owner's GEMM3 then streams the constraint data twice instead of once per 128 columns.
void update_shard_bs(lrn_ctx* c) {
  int bs = 128;
  if (c->shard_bs_opt > 0) bs = c->shard_bs_opt;
  else if (c->world > 1 && c->nvar > 0) {
    int per = (c->nvar + 2 * c->world - 1) / (2 * c->world);
    bs = std::max(128, ((per + 127) / 128) * 128);
  }
  c->shard_bs = bs;
  c->counts["shard_bs"] = bs;
}

int copy_in(lrn_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return LRN_OK;
  if (!src || !dst) return set_error(c, LRN_ERR_ARG, "copy_in: null pointer");
  hipMemcpyKind k = is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  LRN_HIP(c, hipMemcpyAsync(dst, src, bytes, k, c->stream));
  if (k == hipMemcpyHostToDevice) LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

int copy_out(lrn_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return LRN_OK;
  if (!src || !dst) return set_error(c, LRN_ERR_ARG, "copy_out: null pointer");
  hipMemcpyKind k = is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  LRN_HIP(c, hipMemcpyAsync(dst, src, bytes, k, c->stream));
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

int upload(lrn_ctx* c, DBuf& b, const void* src, size_t bytes, size_t alloc_bytes) {
  LRN_TRY(ensure(c, b, std::max(bytes, alloc_bytes)));
  return copy_in(c, b.p, src, bytes);
}

void tic(lrn_ctx* c) {
  if (c->profile) (void)hipEventRecord(c->ev0, c->stream);
}
void toc(lrn_ctx* c, const char* key) {
  if (!c->profile) return;
  (void)hipEventRecord(c->ev1, c->stream);
  (void)hipEventSynchronize(c->ev1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  c->timing[key] += ms;
  c->counts[key] += 1;
}

// (rebuilt on the first use after the next upload of factors)
void drop_rank_classes(LmiBlock& b) {
  for (DBuf* d : b.rank_class_bufs()) release(*d);
  b.rg_ready = false;
  b.Yc_version = -1;
  b.rg_Rc = b.rg_ntiles = 0;
}

// the diagonal parts belong to the declaration "factored": they go with it
void drop_diag(LmiBlock& b) {
  for (DBuf* d : b.diag_bufs()) release(*d);
  b.dg_n = 0;
}

}  // namespace lrn
