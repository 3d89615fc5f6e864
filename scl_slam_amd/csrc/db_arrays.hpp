// db_arrays.hpp -- the per-keyframe arrays of the database (layout: kernels.hpp), described ONCE: a table of what a row of each array
// is, and the struct of the nine typed pointers the table addresses.  Host code only (no HIP): the vector types come in as template
// arguments, so that tests/cpp/ingest_plan_check.cpp can check the table's sizes and offsets without a GPU.  Allocation, the copies of
// rows between two sets and the free are written once over the table in ingest_host.hip; a tenth array is a row here, a member below
// and a line in db_view / query_view / ingest_args.
#pragma once

#include <cstddef>

namespace scl {

// the engine's shape as the row widths see it
struct DbShape { size_t tile, S, R4, hstride, kmask, hkw, halign, RG; };   // tile = RG * S; kmask = 8 words; halign = halign_bytes(S), 0: no image on this grid

struct DbArrayInfo {
    size_t elem_bytes;              // bytes per element
    size_t DbShape::*width;         // elements per row (a keyframe's slot, or a staging row)
    bool staged;                    // has the staging (and mirror) rows behind the database's slots
    bool slot_major;                // [rows][width]; false: [width][cap] -- the tiled ring key, whose row r is column r of `width` lines of cap elements
};

// in the order they are allocated and copied in (the tiled ring key last)
enum DbArrayId { kDbDesc = 0, kDbVkey, kDbNorm, kDbRkey, kDbHdesc, kDbKmask, kDbHkey, kDbHalign, kDbRkey4, kDbArrayCount };

constexpr DbArrayInfo kDbArrays[kDbArrayCount] = {
    {16, &DbShape::tile,    true,  true},    // desc   float4 [rows][RG][S]
    {8,  &DbShape::S,       true,  true},    // vkey   double [rows][S]
    {8,  &DbShape::S,       true,  true},    // norm   double [rows][S]
    {4,  &DbShape::R4,      true,  true},    // rkey   float  [rows][R4]
    {8,  &DbShape::hstride, true,  true},    // hdesc  uint2  [rows][hstride]
    {4,  &DbShape::kmask,   true,  true},    // kmask  u32    [rows][8]
    {2,  &DbShape::hkw,     true,  true},    // hkey   half   [rows][hkw]
    {1,  &DbShape::halign,  false, true},    // halign bytes  [cap][halign_bytes(S)]: a scan is the alignment's other operand, so no staging rows
    {16, &DbShape::RG,      false, false},   // rkey4  float4 [RG][cap]: the top-k scan reads keyframes only
};

inline size_t db_row_bytes(const DbArrayInfo &a, const DbShape &sh) { return a.elem_bytes * (sh.*a.width); }
inline bool db_array_present(const DbArrayInfo &a, const DbShape &sh) { return db_row_bytes(a, sh) != 0; }
inline size_t db_array_rows(const DbArrayInfo &a, size_t cap, size_t stage_rows) { return cap + (a.staged ? stage_rows : 0); }
inline size_t db_array_bytes(const DbArrayInfo &a, const DbShape &sh, size_t cap, size_t stage_rows) { return db_row_bytes(a, sh) * db_array_rows(a, cap, stage_rows); }
// where row `row` begins (staging row j is row cap + j); [width][cap]: its element of the first line, the others a pitch of
// elem_bytes * cap apart
inline size_t db_row_offset(const DbArrayInfo &a, const DbShape &sh, size_t row) { return (a.slot_major ? db_row_bytes(a, sh) : a.elem_bytes) * row; }

// The pointers of one set of arrays.  Kernels and views read the typed members; the table reaches them through at()
template <class F4, class U2> struct DbArraysOf {
    F4 *d_desc = nullptr; double *d_vkey = nullptr; double *d_norm = nullptr; float *d_rkey = nullptr;
    U2 *d_hdesc = nullptr; unsigned int *d_kmask = nullptr; unsigned short *d_hkey = nullptr; unsigned char *d_halign = nullptr;
    F4 *d_rkey4 = nullptr;

    void *at(int id) const
    {
        void *const p[kDbArrayCount] = {d_desc, d_vkey, d_norm, d_rkey, d_hdesc, d_kmask, d_hkey, d_halign, d_rkey4};
        return p[id];
    }
    void set(int id, void *p)
    {
        switch (id) {
        case kDbDesc:   d_desc = static_cast<F4 *>(p); break;
        case kDbVkey:   d_vkey = static_cast<double *>(p); break;
        case kDbNorm:   d_norm = static_cast<double *>(p); break;
        case kDbRkey:   d_rkey = static_cast<float *>(p); break;
        case kDbHdesc:  d_hdesc = static_cast<U2 *>(p); break;
        case kDbKmask:  d_kmask = static_cast<unsigned int *>(p); break;
        case kDbHkey:   d_hkey = static_cast<unsigned short *>(p); break;
        case kDbHalign: d_halign = static_cast<unsigned char *>(p); break;
        case kDbRkey4:  d_rkey4 = static_cast<F4 *>(p); break;
        default: break;
        }
    }
};

}  // namespace scl
