// rowstore_kernels.h -- the kernels of the row store and the row bank (rowstore.cpp).  rs_copy moves a table of contiguous pieces of float32
// elements between the store's three rings (mc rows, ap rows, wave samples) and a caller's blocks; a bank's B sets of rings lie behind one
// another in three arrays and a piece addresses them with its 64-bit element offsets, so the bank's append and fetch are rs_copy too.
// rs_pick (at the end) is the bank's masked read of ap rows.  An append is up to six pieces (three arrays, each split where
// the ring ends) handed over by value; a fetch is a table the host built from the caller's spans (one upload), with pieces that have no source:
// the pads, written as +0.0f -- what `AcousticFeature.silent` holds for mc and ap (numpy.zeros, float32) and `silent_wrapper` for the wave.
// Source and destination of a piece start at any 4-byte alignment, independently (ap rows are 513 floats wide).  A piece is cut at the
// destination's 16-byte boundaries: unit 0 of a piece writes the scalars in front of the first boundary and behind the last whole quad (at most
// six), unit q >= 1 writes quad q - 1 with one 128-bit store, read with one 128-bit load when the source has the destination's residue and as
// four scalars otherwise.  Consecutive lanes take consecutive quads, so a wave's store covers 1 KiB of one row run.  256 units per workgroup,
// the workgroups walk the table's blocks grid-stride.  Plain vector stores only; nothing outside [dst, dst + n) of a piece is written and
// nothing outside [src, src + n) is read.
#pragma once
#include "ry_dev.h"

#define RS_ARRAYS 3
#define RS_INLINE 6
#define RS_UNITS 256

struct RsPiece {
    long long src;           // first element in the source array, -1: a pad (zeros)
    long long dst;           // first element in the destination array
    int n;                   // elements, > 0
    int arr;                 // 0 mc, 1 ap, 2 wave
    int blk0;                // its first block of RS_UNITS units; the pieces' blocks follow one another
    int head;                // elements in front of the destination's first 16-byte boundary (host-computed from the address), <= n
};

struct RsCopyParams {
    const RsPiece* tab;      // the table on the card, or null: `inl`
    int n_pieces, n_blocks;
    const float* src[RS_ARRAYS];
    float* dst[RS_ARRAYS];
    RsPiece inl[RS_INLINE];
};

RY_KERNEL(256) void rs_copy(RsCopyParams p) {
    const int tid = (int)threadIdx.x;
    for (int x = (int)blockIdx.x; x < p.n_blocks; x += (int)gridDim.x) {
        RsPiece e;
        if (p.tab) {
            int lo = 0, hi = p.n_pieces - 1;                        // the last piece with blk0 <= x (every piece has at least one block)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (p.tab[mid].blk0 <= x) lo = mid; else hi = mid - 1;
            }
            e = p.tab[lo];
        } else {
            e = p.inl[0];
#pragma unroll
            for (int i = 1; i < RS_INLINE; ++i)
                if (i < p.n_pieces && p.inl[i].blk0 <= x) e = p.inl[i];
        }
        const int u = (x - e.blk0) * RS_UNITS + tid;
        const int quads = (e.n - e.head) >> 2, tail = e.head + 4 * quads;
        if (u > quads) continue;
        float* d = p.dst[e.arr] + e.dst;
        const bool pad = e.src < 0;
        const float* s = p.src[e.arr] + (pad ? 0 : e.src);
        if (u == 0) {
            for (int i = 0; i < e.head; ++i) d[i] = pad ? 0.f : s[i];
            for (int i = tail; i < e.n; ++i) d[i] = pad ? 0.f : s[i];
            continue;
        }
        const int c = e.head + 4 * (u - 1);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!pad) {
            const bool wide = ((reinterpret_cast<unsigned long long>(s + c) >> 2) & 3) == 0;      // d + c is on a 16-byte boundary
            if (wide) v = ry_ld4(s + c);
            else { v[0] = s[c]; v[1] = s[c + 1]; v[2] = s[c + 2]; v[3] = s[c + 3]; }
        }
        ry_st4(d + c, v);
    }
}

// rs_pick: ap rows out of the bank's rings into a packed block, with the silence mask applied on the way -- ry_rowstore_fetch, ry_mask_rows and
// the slice [k0, k1) in one pass that never writes the full ap window.  A piece is a run of WHOLE rows of `cols` floats and carries the mask
// index of its first row; element i of it belongs to row i / cols.  It is cut as rs_copy cuts: unit 0 writes the scalars in front of the
// destination's first 16-byte boundary and behind the last whole quad, unit q >= 1 writes quad q - 1 with one 128-bit store; a quad that
// straddles two rows (cols = 513: rows start at every alignment) takes each element's mask from its own row.  An element of a pad piece or of
// a row whose mask byte is 0 is +0.0f and its source is not read: a quad is loaded with one 128-bit load only when all four elements are kept
// and the source has the destination's residue.  Plain vector stores only; nothing outside [dst, dst + n) of a piece is written.
struct RsPick {
    long long src;           // first element in the ap array of the bank, -1: a pad (zeros)
    long long dst;           // first element in the packed block
    int n;                   // elements, > 0, a multiple of cols
    int mask0;               // the mask index of its first row
    int blk0;                // its first block of RS_UNITS units
    int head;                // elements in front of the destination's first 16-byte boundary, <= n
};

struct RsPickParams {
    const RsPick* tab;
    int n_pieces, n_blocks, cols;
    const float* src;
    const unsigned char* mask;
    float* dst;
};

RY_KERNEL(256) void rs_pick(RsPickParams p) {
    const int tid = (int)threadIdx.x;
    for (int x = (int)blockIdx.x; x < p.n_blocks; x += (int)gridDim.x) {
        int lo = 0, hi = p.n_pieces - 1;                            // the last piece with blk0 <= x
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.tab[mid].blk0 <= x) lo = mid; else hi = mid - 1;
        }
        const RsPick e = p.tab[lo];
        const int u = (x - e.blk0) * RS_UNITS + tid;
        const int quads = (e.n - e.head) >> 2, tail = e.head + 4 * quads;
        if (u > quads) continue;
        float* d = p.dst + e.dst;
        const bool pad = e.src < 0;
        const float* s = p.src + (pad ? 0 : e.src);
        const unsigned char* m = p.mask + e.mask0;
        if (u == 0) {
            for (int i = 0; i < e.head; ++i) d[i] = (!pad && m[i / p.cols] != 0) ? s[i] : 0.f;
            for (int i = tail; i < e.n; ++i) d[i] = (!pad && m[i / p.cols] != 0) ? s[i] : 0.f;
            continue;
        }
        const int c = e.head + 4 * (u - 1);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!pad) {
            int row = c / p.cols, at = c - row * p.cols;
            bool k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                k[j] = m[row] != 0;
                if (++at == p.cols) { at = 0; ++row; }
            }
            const bool wide = ((reinterpret_cast<unsigned long long>(s + c) >> 2) & 3) == 0;      // d + c is on a 16-byte boundary
            if (wide && k[0] && k[1] && k[2] && k[3]) v = ry_ld4(s + c);
            else {
                if (k[0]) v[0] = s[c];
                if (k[1]) v[1] = s[c + 1];
                if (k[2]) v[2] = s[c + 2];
                if (k[3]) v[3] = s[c + 3];
            }
        }
        ry_st4(d + c, v);
    }
}
