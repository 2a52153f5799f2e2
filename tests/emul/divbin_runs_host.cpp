// Host harness of the run-table builder of the fused divergence + binning launch (orphics_amd/csrc/divbin_runs.hpp): a C entry for
// tests/test_divbin_runs_host.py, and -- built with -DDIVBIN_RUNS_MAIN -- a stand-alone program that runs the builder over a radial
// and a checkerboard plane (the form to put under a sanitizer).
#include "../../orphics_amd/csrc/divbin_runs.hpp"
#include <cstdio>
#include <cstring>

extern "C" {
// ids_t: [tiles][rows][1 << logc].  Returns -1 (no run table) or the number of entries; when the buffers are large enough
// (ent_cap entries; off: tiles * (nids + 1)) they are filled.
long divbin_runs_build(const int32_t* ids_t, int tiles, int rows, int logc, int width, int rband, int nids, int nxh, int max_entries, uint64_t* ent,
                       long ent_cap, int32_t* off) {
    oa::DivRunTable t;
    if (!oa::divbin_build_runs(ids_t, tiles, rows, logc, width, rband, nids, nxh, max_entries, &t)) return -1;
    if (ent && (long)t.ent.size() <= ent_cap) std::memcpy(ent, t.ent.data(), t.ent.size() * sizeof(uint64_t));
    if (off) std::memcpy(off, t.off.data(), t.off.size() * sizeof(int32_t));
    return (long)t.ent.size();
}
}

#ifdef DIVBIN_RUNS_MAIN
int main() {
    const int rows = 256, logc = 2, C = 1 << logc, nxh = 128, width = 129, tiles = (width + C - 1) / C, nids = 21;
    std::vector<int32_t> ids((size_t)tiles * rows * C);
    for (int chk = 0; chk < 2; ++chk) {
        for (int t = 0; t < tiles; ++t)
            for (int y = 0; y < rows; ++y)
                for (int c = 0; c < C; ++c) {
                    const long x = (long)t * C + c, ky = y < rows / 2 ? y : y - rows;
                    long r2 = x * x + ky * ky, r = 0;
                    while ((r + 1) * (r + 1) <= r2) ++r;
                    ids[((size_t)t * rows + y) * C + c] = chk ? (int32_t)((x + y) & 1) : (int32_t)(r / 8 < nids ? r / 8 : nids);
                }
        oa::DivRunTable tab;
        const bool ok = oa::divbin_build_runs(ids.data(), tiles, rows, logc, width, 100, nids, nxh, 2 * (rows * C / 16), &tab);
        std::printf("%s: %s, %zu entries\n", chk ? "checkerboard" : "radial", ok ? "table" : "no table", tab.ent.size());
        if (ok == (chk != 0)) return 1;
    }
    return 0;
}
#endif
