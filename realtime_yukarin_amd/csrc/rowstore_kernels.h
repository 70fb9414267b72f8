// rowstore_kernels.h -- the one kernel of the row store (rowstore.cpp): rs_copy moves a table of contiguous pieces of float32 elements between
// the store's three rings (mc rows, ap rows, wave samples) and a caller's blocks.  An append is up to six pieces (three arrays, each split where
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
