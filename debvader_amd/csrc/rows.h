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
  template <typename T>                                 // (an input column the kernels only read)
  void add(const T*& dev, const T* host, size_t elems) {
    cols[ncols++] = Column{(void**)&dev, (char*)const_cast<T*>(host), elems * sizeof(T)};
  }
  size_t bytes() const;                                 // per galaxy
  int alloc(int64_t n);                                 // device memory for n rows: every column's device pointer at its row 0
  void advance(int64_t r);                              // every device pointer r rows on (the view that starts at row r)
  int upload(int64_t r, int64_t n, hipStream_t s) const;     // host rows [r, r + n) to device rows [0, n)
  int download(int64_t r, int64_t n, hipStream_t s) const;   // device rows [0, n) to host rows [r, r + n)
};

// Host staging for rows that are computed in another order than the caller's: take() gives every column of r that has a host
// array n staged rows and makes them the column's host, add() stages a host-only column and returns its rows;
// scatter() copies staged row k to row rowmap[k] of every caller's array.
struct RowStage {
  struct Col { char* dest; size_t width; std::vector<char> rows; };
  Col cols[Rows::MAX_COLS];
  int ncols = 0;
  void* add(void* dest, size_t width, int64_t n);
  void take(Rows& r, int64_t n);
  void scatter(const int* rowmap, int64_t n) const;
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
void fitflux_columns(Rows& r, FitFluxRows& dev, const FitFluxRows& host, int nb, bool weighted, bool nonneg);

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

// The cut of M fields into runs of consecutive WHOLE fields (no HIP call): run k is the fields first[k] .. first[k + 1] - 1.  A
// run takes fields while its bytes - row_bytes per row, field_bytes per field - stay within `budget`, its fields within
// max_fields and its rows within max_stamps (either 0: no cap); it always holds at least one field.  Returns -1, or the field
// that exceeds the budget alone, with its bytes in *need.
struct FieldRuns {
  std::vector<int> first{0};
  size_t max_rows = 0, max_fields = 0;                  // of the largest run
};
int plan_field_runs(const int64_t* field_ptr, int M, size_t row_bytes, size_t field_bytes, size_t budget, int64_t max_stamps,
                    int64_t max_fields, FieldRuns* runs, size_t* need);

// The joint order of the rows of a resident field set (no HIP call).  The set holds its rows pass after pass;
// pass_fptr[p][f] is the first row of field f counted from row 0 of kept pass p, pass_fptr[p][M] the rows of the pass.  The
// joint order goes field by field, pass ascending inside a field, then the in-pass order: joint row k is resident row
// rowmap[k] and lies in field sfield[k]; fptr32 / fptr64 [M + 1] are the joint field_ptr.  This is what fit_group indexes and
// what decides which copy of a twin stamp is dropped.  places(): the resident placements [.][2] gathered into joint order.
struct JointOrder {
  std::vector<int> rowmap, sfield, fptr32;
  std::vector<int64_t> fptr64;
  std::vector<int32_t> places(const int32_t* resident) const;
};
JointOrder joint_order(const std::vector<std::vector<int>>& pass_fptr, int M);

// The host side of a call that reads the stamps of complete fields against the fields (flux fit, moments on the fields): the
// field stacks [M][F][F][nb], any of them null; the bytes the caller allocates beside the walker's - per row, per field, and
// `fixed` once; empty_runs: a run without rows is visited too (the sky fit solves fields that hold no galaxy).  The walker
// sets max_rows / max_fields, the largest run, before the first body call: what the body allocates is sized by them.
struct WholeFields {
  const double *model_h, *data_h, *weight_h;
  size_t row_bytes, field_bytes, fixed;
  bool empty_runs;
  size_t max_rows = 0, max_fields = 0;
};

// Fields [0, M) a run of whole fields at a time (plan_field_runs within half of free device memory less f.fixed, and within
// dv_debug_scene_limits in the development build; a field that does not fit alone is refused with E_NOMEM).  `in` holds the
// per-row inputs - the stamps and placements are columns at v.stamps / v.places - and `out` the rows; v carries cs, nb and F.
// The walker allocates both, the field of every row, the run's field_ptr and the stacks for the largest run, and per run
// uploads them, points v at them (f0 = 0: rows and fields count from the run's first), runs body(v, fa, nf, r0, fptr_h) for the
// nf fields from fa, whose first row is r0 and whose rows fptr_h [nf + 1] counts from r0, downloads out to host rows r0 .. and
// waits.  A failure waits for the stream before any buffer of the caller goes.
int walk_whole_fields(const char* who, int M, const int64_t* field_ptr, int64_t N, WholeFields& f, FieldStamps& v, Rows& in,
                      Rows& out, hipStream_t s,
                      const std::function<int(const FieldStamps& v, int fa, int nf, int64_t r0, const int* fptr_h)>& body);

}  // namespace dv
