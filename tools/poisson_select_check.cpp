// poisson_select_check.cpp -- the pressure solver's selection (csrc/poisson_select.h) exercised on the host: no device, no HIP call.
//
// For every shape at which the single-device solver takes another pipeline, with and without each OCN_POISSON_* switch, this builds the
// choice and the three pass lists, checks their invariants and prints the pass names.  Meant to be built with the host sanitizers:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Ioceananigans.jl_amd/csrc \
//         tools/poisson_select_check.cpp -o tools/bin/poisson_select_check && tools/bin/poisson_select_check
//
// Exit status 0 iff every invariant holds and every pass name occurs in at least one list.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "poisson_select.h"

using namespace ocn::poisson;

static bool col_ok(int N) { return N == 64 || N == 128 || N == 256 || N == 512; }     // csrc/colfft.hip colfft_supported
static bool row_ok(int N) { return N == 128 || N == 256 || N == 512 || N == 1024; }   // csrc/rowfft.hip rowfft_supported

struct Row {
    const char *topo;   // one letter per direction: P, B, F
    int N[3];
    bool stretched_z;
    int tdim;           // 2, or the stretched x (0) / y (1)
    const char *env;    // a switch "NAME=V", or ""
};

static const Row ROWS[] = {
    {"PPP", {16, 16, 16}, false, 2, ""}, {"PPP", {16, 16, 64}, false, 2, ""}, {"PPP", {128, 64, 64}, false, 2, ""}, {"PPF", {16, 16, 1}, false, 2, ""},
    {"PPB", {16, 16, 16}, false, 2, ""}, {"PPB", {16, 16, 16}, true, 2, ""}, {"PPB", {128, 64, 64}, false, 2, ""}, {"PPB", {128, 64, 16}, false, 2, ""},
    {"PPB", {128, 64, 64}, true, 2, ""},
    {"BBB", {7, 7, 7}, false, 2, ""}, {"BBB", {16, 16, 16}, false, 2, ""}, {"BBB", {64, 64, 64}, false, 2, ""}, {"BBB", {64, 64, 16}, true, 2, ""},
    {"BBF", {64, 64, 1}, false, 2, ""}, {"PBB", {16, 16, 16}, false, 2, ""}, {"PBB", {64, 64, 64}, false, 2, ""}, {"PBB", {16, 16, 16}, true, 2, ""},
    {"PBP", {16, 64, 16}, false, 2, ""}, {"BPB", {16, 64, 64}, false, 2, ""}, {"BPP", {16, 16, 16}, false, 2, ""}, {"PBF", {128, 6, 1}, false, 2, ""},
    {"PPP", {16, 16, 16}, false, 2, "OCN_POISSON_GENERAL=1"},
    {"BPP", {16, 16, 16}, false, 0, ""}, {"PBP", {16, 16, 16}, false, 1, ""}, {"BBB", {64, 64, 64}, false, 0, ""},
    {"PPP", {16, 16, 16}, false, 2, "OCN_POISSON_C2C=1"}, {"PPB", {16, 16, 16}, false, 2, "OCN_POISSON_C2C=1"},
    {"PPP", {16, 16, 16}, false, 2, "OCN_POISSON_DIRECT_OUT=0"}, {"PPP", {16, 16, 64}, false, 2, "OCN_POISSON_FUSED_Z=0"},
    {"PPP", {128, 64, 64}, false, 2, "OCN_POISSON_CUSTOM_XY=0"}, {"PPB", {128, 64, 16}, false, 2, "OCN_POISSON_CUSTOM_XY=0"},
    {"PPB", {128, 64, 64}, false, 2, "OCN_POISSON_DCT_Z=0"}, {"PPP", {16, 16, 16}, false, 2, "OCN_POISSON_SOURCE_WRAP=0"},
    {"PPB", {16, 16, 16}, false, 2, "OCN_POISSON_GENERAL=1"}, {"BBB", {16, 16, 16}, false, 2, "OCN_POISSON_GENERAL_TRI=1"},
    {"BBB", {7, 7, 7}, false, 2, "OCN_POISSON_NAIVE_DCT=1"}, {"PBB", {16, 16, 16}, false, 2, "OCN_POISSON_PACKED=0"},
    {"BBB", {16, 16, 16}, false, 2, "OCN_POISSON_PACKED=0"}, {"BBB", {64, 64, 64}, false, 2, "OCN_POISSON_GENERAL_COLFFT=0"},
    {"BBB", {64, 64, 64}, false, 2, "OCN_POISSON_FUSED_DCT=0"}, {"BPB", {16, 64, 64}, false, 2, "OCN_POISSON_FUSED_DCT=0"},
    {"BBB", {64, 64, 64}, false, 2, "OCN_POISSON_ROW_DCT=0"}, {"PBB", {64, 64, 64}, false, 2, "OCN_POISSON_ROW_DCT=0"},
    {"BBB", {16, 16, 16}, false, 2, "OCN_POISSON_FUSE_SHUFFLES=0"}, {"BBB", {64, 64, 64}, false, 2, "OCN_POISSON_DCT_TO_FIELD=0"},
};

static int topo_code(char c) { return c == 'P' ? OCN_PERIODIC : c == 'B' ? OCN_BOUNDED : OCN_FLAT; }

static int failures = 0;
#define EXPECT(cond, ...)                                    \
    do {                                                     \
        if (!(cond)) {                                       \
            ++failures;                                      \
            std::printf("  FAILED %s: ", #cond);             \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
        }                                                    \
    } while (0)

static std::string names(const std::vector<PassRec> &l, std::set<int> &seen)
{
    std::string s;
    for (const PassRec &r : l) {
        seen.insert((int)r.pass);
        s += s.empty() ? "" : " ";
        s += pass_name(r.pass);
        if (r.pass == Pass::ColumnFFT || r.pass == Pass::ColumnDCT || r.pass == Pass::LineFFT || r.pass == Pass::Shuffle || r.pass == Pass::RowPair ||
            r.pass == Pass::NaiveTransform || r.pass == Pass::RowDCT || r.pass == Pass::ColumnDCTToField)
            s += "(" + std::string(1, "xyz"[r.d]) + "," + std::to_string(r.mode) + ")";
        if (r.pass == Pass::TwiddlePermute) s += "(" + std::string(1, "xyz"[r.d]) + "," + std::string(1, "xyz"[r.d2]) + ")";
    }
    return s;
}

int main()
{
    std::set<int> seen;
    double dummy = 1.0;  // (a stretched z is a non-NULL dzc; the selection never follows the pointer)
    for (const Row &row : ROWS) {
        std::string name, value;
        if (row.env[0]) {
            const char *eq = std::strchr(row.env, '=');
            name.assign(row.env, eq - row.env);
            value = eq + 1;
            setenv(name.c_str(), value.c_str(), 1);
        }
        ocn_grid g{};
        g.Nx = row.N[0]; g.Ny = row.N[1]; g.Nz = row.N[2];
        g.Hx = g.Hy = g.Hz = 3;
        g.tx = topo_code(row.topo[0]); g.ty = topo_code(row.topo[1]); g.tz = topo_code(row.topo[2]);
        g.Lx = 1.0; g.Ly = 2.5; g.Lz = 4.0;
        g.dx = g.Lx / g.Nx; g.dy = g.Ly / g.Ny; g.dz = g.Lz / g.Nz;
        if (row.stretched_z) g.dzc = g.dzf = &dummy;
        // (ocn_poisson_create's routing)
        const bool general = row.tdim != 2 || g.tx != OCN_PERIODIC || g.ty != OCN_PERIODIC || (env_set("OCN_POISSON_GENERAL") && !g.dzc);
        for (int retry = 0; retry < 2; ++retry) {  // the plain attempt and the one after a failed plan self test
            const PoissonChoice c = general ? choose_general(g, row.tdim, retry == 0, col_ok) : choose_periodic(g, retry == 0, col_ok, row_ok);
            const PassLists L = build_passes(c);
            if (retry == 0) {
                std::printf("%s %dx%dx%d%s%s %s: info (%d, %d, %d)\n  source: ", row.topo, row.N[0], row.N[1], row.N[2], row.stretched_z ? " stretched z" : "",
                            row.tdim == 0 ? " stretched x" : row.tdim == 1 ? " stretched y" : "", row.env, c.info_kind(), c.info_r2c(), c.info_direct_out());
                std::printf("%s\n  set:    ", names(L.source, seen).c_str());
                std::printf("%s\n  solve:  ", names(L.set_source, seen).c_str());
                std::printf("%s\n", names(L.solve, seen).c_str());
            }
            // ---- invariants
            EXPECT(L.source.size() == 1 && L.set_source.size() == 1 && !L.solve.empty(), "list sizes %zu %zu %zu", L.source.size(), L.set_source.size(), L.solve.size());
            const Pass last = L.solve.back().pass;
            EXPECT(last == Pass::CopyReal || last == Pass::ColumnDCTToField || last == Pass::RowFFTToField || last == Pass::FFTRealInverseToField ||
                       last == Pass::FFTRealInverseAndCopy, "a solve ends in the pressure field, not in %s", pass_name(last));
            int skips = 0;
            for (const PassRec &r : L.solve) {
                skips += r.skip_if_gathered;
                EXPECT(r.d >= 0 && r.d < 3 && r.d2 >= -1 && r.d2 < 3, "direction out of range in %s", pass_name(r.pass));
                EXPECT(r.n[0] >= 1 && r.n[1] >= 1 && r.n[2] >= 1, "empty extents in %s", pass_name(r.pass));
                EXPECT((long long)r.n[0] * r.n[1] * r.n[2] <= (long long)g.Nx * g.Ny * g.Nz, "%s sees more than the grid's elements", pass_name(r.pass));
                if (r.pass == Pass::ColumnFFT || r.pass == Pass::ColumnDCT || r.pass == Pass::ColumnDCTToField || r.pass == Pass::ColumnFFTSolve ||
                    r.pass == Pass::ColumnDCTSolve)
                    EXPECT(r.d >= 1 && col_ok(r.n[r.d]), "column kernel on length %d along %d", r.n[r.d], r.d);
                if (r.pass == Pass::RowDCT) EXPECT(col_ok(g.Nx) && g.Ny % 2 == 0, "row kernel on %d x %d", g.Nx, g.Ny);
                if (r.pass == Pass::LineFFT) EXPECT(c.lines[r.d], "rocFFT lines along %d without a plan", r.d);
                if (r.pass == Pass::RowFFTToField || r.pass == Pass::RowFFTOfRealSource) EXPECT(row_ok(g.Nx), "row FFT kernel on %d", g.Nx);
            }
            // the source pass gathers along a direction iff the solve opens with the gather it replaces
            EXPECT(skips == (L.source[0].d2 >= 0 ? 1 : 0), "%d skippable gathers for source direction %d", skips, L.source[0].d2);
            if (retry == 1) EXPECT(c.general ? !c.packed : c.c2c, "the retry must not choose the plans that failed");
        }
        if (row.env[0]) unsetenv(name.c_str());
    }
    for (int p = 0; p < (int)Pass::Count_; ++p) EXPECT(seen.count(p), "no row reaches pass %s", pass_name((Pass)p));
    std::printf("%s: %zu rows, %zu of %d pass names reached, %d failures\n", failures ? "FAILED" : "ok", sizeof(ROWS) / sizeof(ROWS[0]), seen.size(),
                (int)Pass::Count_, failures);
    return failures ? 1 : 0;
}
