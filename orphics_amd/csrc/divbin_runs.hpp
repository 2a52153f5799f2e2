// Run table of the fused divergence + binning launch (DivRunTail, fft_divbin.hpp).  Plain C++, host only: built once per binding
// from the tile-major copy of the bin ids (ensure_div_tables, pipeline.hip), so that the kernel never reads an id.
//
// In each column the bin id is piecewise constant in the row index (radial bins: one run on the ky >= 0 side, one on the ky < 0
// side per bin).  Per tile of the launch the ids of the kept coarse rows of every column are run-length encoded in the kernel's row
// numbering (coarse row y of the [tile][y][C] layout); runs longer than DIVRUN_MAX_LEN rows are cut, runs whose id lies outside
// [0, nids) or whose column carries no weight (beyond nx / 2, or beyond the band) are dropped.  A tile's entries are sorted by
// (id, column, first row): the entries of one id are a contiguous range, given by the offset list.
//
// Nothing here knows about bin edges: any id plane works.  A tile with more than `max_entries` runs (ids that are not piecewise
// constant, a checkerboard) makes the whole binding "no run table" and the launch keeps the id-reading tail.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace oa {

constexpr int DIVRUN_MAX_LEN = 64;

// one entry, 8 bytes: low word = first row (16 bits) | length << 16 (8 bits) | column in tile << 24; high word = id
inline uint64_t divrun_pack(int col, int first, int len, int id) {
    return (uint64_t)((uint32_t)first | ((uint32_t)len << 16) | ((uint32_t)col << 24)) | ((uint64_t)(uint32_t)id << 32);
}
inline int divrun_first(uint64_t e) { return (int)(e & 0xffffu); }
inline int divrun_len(uint64_t e) { return (int)((e >> 16) & 0xffu); }
inline int divrun_col(uint64_t e) { return (int)((e >> 24) & 0xffu); }
inline int divrun_id(uint64_t e) { return (int)(uint32_t)(e >> 32); }

struct DivRunTable {
    std::vector<uint64_t> ent;      // all tiles' entries, tile after tile
    std::vector<int32_t> off;       // [tiles][nids + 1]: entries of id i of tile t are ent[off[t][i] .. off[t][i + 1]) (absolute indices)
};

// ids_t: [tiles][rows][1 << logc] (pack_tiles' layout).  width: columns of the band (column tile * C + c is kept when < width);
// rband > 0: rows rband <= y <= rows - rband are not kept (ColDivArgs::rband on the coarse grid); nxh = nx / 2.
// Returns false -- and an empty table -- when a tile needs more than max_entries entries or the shape does not fit an entry.
inline bool divbin_build_runs(const int32_t* ids_t, int tiles, int rows, int logc, int width, int rband, int nids, int nxh, int max_entries,
                              DivRunTable* out) {
    out->ent.clear();
    out->off.clear();
    if (tiles < 1 || rows < 1 || rows > 0x10000 || logc < 0 || logc > 8 || nids < 1) return false;
    const int C = 1 << logc;
    out->off.reserve((size_t)tiles * (nids + 1));
    std::vector<uint64_t> runs;                  // this tile's entries in (column, first row) order
    std::vector<int32_t> cnt((size_t)nids + 1);
    for (int t = 0; t < tiles; ++t) {
        runs.clear();
        const int32_t* tid = ids_t + (size_t)t * rows * C;
        for (int c = 0; c < C; ++c) {
            const long col = (long)t * C + c;
            if (col >= width || col > nxh) continue;
            int first = 0, len = 0, cur = -1;
            for (int y = 0; y <= rows; ++y) {
                const bool kept = y < rows && !(rband > 0 && y >= rband && y <= rows - rband);
                const int id = kept ? tid[(size_t)y * C + c] : -1;
                const bool valid = id >= 0 && id < nids;
                if (len > 0 && valid && id == cur && len < DIVRUN_MAX_LEN) { ++len; continue; }
                if (len > 0) runs.push_back(divrun_pack(c, first, len, cur));
                len = 0;
                if (valid) { first = y; len = 1; cur = id; }
            }
        }
        if ((long)runs.size() > (long)max_entries) {
            out->ent.clear();
            out->off.clear();
            return false;
        }
        // stable counting sort by id: (column, first row) order survives inside each id
        for (int i = 0; i <= nids; ++i) cnt[i] = 0;
        for (uint64_t e : runs) ++cnt[divrun_id(e) + 1];
        const int32_t base = (int32_t)out->ent.size();
        for (int i = 0; i < nids; ++i) cnt[i + 1] += cnt[i];
        for (int i = 0; i <= nids; ++i) out->off.push_back(base + cnt[i]);
        out->ent.resize((size_t)base + runs.size());
        for (uint64_t e : runs) out->ent[(size_t)base + cnt[divrun_id(e)]++] = e;
    }
    return true;
}

}  // namespace oa
