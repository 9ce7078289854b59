// Per-galaxy row sets of the catalogue calls (host code only): a row set states its columns once, and what is
// done with rows - allocate, address row r, upload, download, count bytes - is derived from that list here.
#pragma once
#include "common.h"

#include <functional>

namespace dv {

// One column: `width` bytes per galaxy, in device memory at *dev (the pointer the kernels are given: a member of the row
// set's kernel-facing struct, or a local of the call) and in the caller's array `host`.  host null: the column lives on the
// device alone (scratch, or rows the call copies itself).
struct Column {
  void** dev;
  char* host;
  size_t width;
};

// The columns of one row set - or of the inputs of a stand-alone call - and, once alloc() has run, the device memory behind
// them.  A column the call does not have is not added: its device pointer stays null.
struct Rows {
  static constexpr int MAX_COLS = 16;
  Column cols[MAX_COLS];
  int ncols = 0;
  DevBuf<char> mem[MAX_COLS];                            // one allocation per column
  template <typename T>
  void add(T*& dev, const T* host, size_t elems) {
    cols[ncols++] = Column{(void**)&dev, (char*)const_cast<T*>(host), elems * sizeof(T)};
  }
  template <typename T>
  void add(T*& dev, std::nullptr_t, size_t elems) { add(dev, (const T*)nullptr, elems); }
  size_t bytes() const;                                 // per galaxy
  int alloc(int64_t n);                                 // device memory for n rows: every column's device pointer at its row 0
  void advance(int64_t r);                              // every device pointer r rows on (the view that starts at row r)
  int upload(int64_t r, int64_t n, hipStream_t s) const;     // host rows [r, r + n) to device rows [0, n)
  int download(int64_t r, int64_t n, hipStream_t s) const;   // device rows [0, n) to host rows [r, r + n)
};

// The columns of the row sets, each stated once, in the file of its kernels: `dev` is where the device pointers are
// kept (alloc() sets them; a caller with rows of its own sets them itself), `host` the caller's arrays - all null for rows
// that stay on the device.  The scratch rows of a Monte-Carlo pass (`reps` rows per galaxy) are never copied.
void catalogue_columns(Rows& r, CatRows& dev, const CatRows& host, int nb, bool err);
void mc_columns(Rows& r, McState& dev, const McState& host, int nb, int S, bool keep);
void mc_scratch_columns(Rows& r, McScratch& dev, int nb, int reps);
void blend_columns(Rows& r, BlendRows& dev, const BlendRows& host);
void regauss_columns(Rows& r, RegaussRows& dev, const RegaussRows& host);
void aperture_columns(Rows& r, ApertureRows& dev, const ApertureRows& host, const ApertureParams& p, int nb, bool err);
void aperture_field_columns(Rows& r, ApertureFieldRows& dev, const ApertureFieldRows& host, const ApertureParams& p, int nb);
void moments_field_columns(Rows& r, MomentsFieldRows& dev, const MomentsFieldRows& host, int nb);
void fitflux_columns(Rows& r, FitFluxRows& dev, const FitFluxRows& host, int nb, bool weighted = false, bool nonneg = false);

// The refusals every field-grouped call takes for its tables, before any GPU work, and the tables: N < 2^31 `noun`s, F within
// 1 .. 32768 (F null: the caller has its own bound), field_ptr from 0 to N and never decreasing, every placement within
// +-2^28 (places null: none given); sfield[i] = the field of row i, fptr32 = field_ptr as the kernels read it (either null:
// not wanted).
int place_check(const char* who, int64_t i, const int32_t* places);
int field_tables(const char* who, const char* noun, int M, const int64_t* field_ptr, int64_t N, const int* F,
                 const int32_t* places, std::vector<int32_t>* sfield, std::vector<int>* fptr32);

// The rows and fields a stand-alone call holds on the device at a time: 1 / `share` of free device memory, less `fixed`
// bytes, for rows of row_bytes; with field_bytes > 0 the same share for fields.  Both at least 1; the development build takes
// the minimum with dv_debug_scene_limits.
int scene_limits(int share, size_t fixed, size_t row_bytes, size_t field_bytes, int64_t* chunk, int64_t* gmax);

// Rows [0, N) at most `chunk` at a time (half of free device memory less `fixed`, at most max_rows): the walker allocates
// `in` and `out` for a chunk, and per chunk uploads in, runs body(base, n) for rows [base, base + n), downloads out and waits.
// A failure waits for the stream before any buffer of the caller goes.
int walk_rows(int64_t N, int64_t max_rows, size_t fixed, Rows& in, Rows& out, hipStream_t s,
              const std::function<int(int64_t base, int n)>& body);

// The model and optional data fields of a field-grouped call: host stacks [M][felems], and the device copies of the chunk's
// fields (the walker sets them: field fa of the chunk first; data_d null without data_h)
struct FieldStacks {
  const double *model_h, *data_h;
  size_t felems;
  int M;
  double *model_d = nullptr, *data_d = nullptr;
};

// The same for rows grouped by field (sfield [N] ascending): at most `chunk` rows of at most `gmax` consecutive fields at a
// time - a quarter of free device memory for the rows, a quarter for the fields - with those fields uploaded beside the rows;
// body(base, n, fa) gets the chunk's first field.
int walk_field_rows(int64_t N, const int32_t* sfield, FieldStacks& f, Rows& in, Rows& out, hipStream_t s,
                    const std::function<int(int64_t base, int n, int fa)>& body);

}  // namespace dv
