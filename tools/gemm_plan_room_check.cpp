// Stand-alone check that the room of the matrix route follows from its plans: over a grid of table shapes, every combination
// of the five switches and both tail modes (mkb_pool_step, whose products fold their tails, and mkb_pool_score_fwd / _bwd),
// every product of the plan writes inside the workspace segment carve() gives it -- the scores inside the caller's [B, P], the
// dQ slices, ks * M * ld floats of split-K partials --, the segments do not overlap, and the layout is no larger than what
// mkb_pool_step_workspace_bytes reports with the environment unset.  The workspace is a fake non-null base pointer: nothing is
// dereferenced, nothing is launched, no device is needed.  It also puts the formula the partial buffer had before it was taken
// from the plans (8 * B * max(P, De) floats) through the same check at three shapes, where it must come out too small.
// Built with the host sanitizers, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/gemm_plan_room_check.cpp \
//       -o /tmp/gemm_plan_room_check && /tmp/gemm_plan_room_check
#include "../mkb_amd/csrc/score_pool.hip"  // plan_pool and carve are internal to this translation unit

#include <vector>

// What score_pool.hip calls in the library's other translation units.  Nothing is launched here, so they are not linked in.
namespace mkb {
int set_error(int code, const char *, ...) { return code; }
ProfScope::ProfScope(int kind, hipStream_t st) : kind(kind), st(st), slot(-1) {}
ProfScope::~ProfScope() {}
int adversarial_launch(const float *, const float *, const float *, const uint16_t *, int64_t, int64_t, float, const float *, float *, float *,
                       float *, float *, hipStream_t, RowLoss *, SeedLayout, const GemmTail *, int *, const int64_t *, const int64_t *) { return MKB_ERR_INVALID; }
template <int MODEL, bool HEAD>
int pool_launch(int, const PoolPlan &, const PoolArgs &, hipStream_t) { return MKB_ERR_INVALID; }
}  // namespace mkb

static long failures = 0, plans = 0, products = 0;

#define EXPECT(cond, ...)                                \
    do {                                                 \
        if (!(cond)) {                                   \
            if (++failures <= 20) { printf("FAIL " __VA_ARGS__); printf("  [%s]\n", #cond); } \
        }                                                \
    } while (0)

static void set_switch(const char *name, const char *value) {
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}

struct Cell { int model; int d; int64_t B, K; int n_rel; uintptr_t ent; };

static mkb_tables_t tables(const Cell &c) {
    const int64_t de = (c.model == MKB_ROTATE || c.model == MKB_COMPLEX) ? 2 * c.d : c.d, dr = c.model == MKB_COMPLEX ? 2 * c.d : c.d;
    return mkb_tables_t{c.model, c.d, 14541, c.n_rel, de, dr, (const float *)c.ent, (const float *)0x50000000, (const float *)0x50100000, 12.f, 0.5f};
}

// the extents the plan's products write, against the segments of one carved layout
static void check_layout(const Cell &c, const PoolPlan &L, const char *what, int64_t reported) {
    const mkb_tables_t tb = tables(c);
    const int64_t B = c.B, P = 2 * c.K, De = tb.entity_dim;
    unsigned char *base = (unsigned char *)0x10000000;
    const Workspace w = carve(base, B, P, De, L);
    ++plans;
    // the segments in carve()'s order: each ends where the next begins, the last at base + bytes
    const unsigned char *seg[] = {(unsigned char *)w.Q, (unsigned char *)w.dQ, (unsigned char *)w.G, (unsigned char *)w.dpos,
                                  (unsigned char *)w.scratch, (unsigned char *)w.gemm_part, (unsigned char *)w.dXp,
                                  (unsigned char *)w.xused, (unsigned char *)w.rel_rep, (unsigned char *)w.occ,
                                  (unsigned char *)w.depth, (unsigned char *)w.tile_part, base + w.bytes};
    EXPECT(seg[0] == base, "%s model %d d %d B %lld K %lld: Q is not at the base\n", what, c.model, c.d, (long long)B, (long long)c.K);
    for (int i = 0; i + 1 < 13; ++i)
        EXPECT(seg[i] <= seg[i + 1], "%s model %d d %d B %lld K %lld: segment %d overlaps the next\n", what, c.model, c.d, (long long)B, (long long)c.K, i);
    EXPECT((int64_t)w.bytes <= reported, "%s model %d d %d B %lld K %lld: layout %zu bytes > reported %lld\n", what, c.model, c.d,
           (long long)B, (long long)c.K, w.bytes, (long long)reported);
    auto room = [&](int i) { return (size_t)(seg[i + 1] - seg[i]); };
    EXPECT(room(0) >= (size_t)B * De * 4, "%s: Q\n", what);
    EXPECT(room(1) >= (size_t)L.dq_parts * B * De * 4, "%s model %d d %d B %lld K %lld: %d dQ slices\n", what, c.model, c.d, (long long)B,
           (long long)c.K, L.dq_parts);
    EXPECT(room(2) >= (size_t)B * P * 4, "%s: G\n", what);
    if (!L.matrix()) return;
    EXPECT(L.fwd == FwdRoute::Matrix, "%s: a matrix backward without the matrix forward\n", what);
    auto product = [&](const GemmPlan &g, const char *name, size_t c_floats, size_t c_room_bytes) {
        ++products;
        // C itself (one [M][ldc], or the caller's slices), then the partial buffer
        const size_t c_written = g.dest == GemmDest::Partials ? 0 : (size_t)g.slices() * g.s.M * g.s.ldc;
        EXPECT(c_written <= c_floats && c_written * 4 <= c_room_bytes, "%s model %d d %d B %lld K %lld: %s writes %zu floats of C, room %zu\n",
               what, c.model, c.d, (long long)B, (long long)c.K, name, c_written, c_floats);
        const size_t ld = g.tail == GemmTailKind::Scatter ? (size_t)g.s.N : (size_t)g.s.ldc;
        EXPECT(g.part_floats == (g.dest == GemmDest::Partials ? (size_t)g.ks * g.s.M * ld : 0), "%s: %s part_floats\n", what, name);
        EXPECT(g.part_floats <= g.part_bound, "%s: %s writes more than its bound\n", what, name);
        EXPECT(g.part_floats * 4 <= room(5), "%s model %d d %d B %lld K %lld: %s writes %zu bytes of partials, room %zu\n", what, c.model,
               c.d, (long long)B, (long long)c.K, name, g.part_floats * 4, room(5));
        EXPECT(g.tail_handed ? g.tail != GemmTailKind::None : true, "%s: %s hands on no tail\n", what, name);
    };
    product(L.gemm, "S", (size_t)B * P, (size_t)B * P * 4);                       // the caller's pool_score [B, P]
    product(L.products.dq, "dQ", (size_t)L.dq_parts * B * De, room(1));
    // the scattered product's C is the table gradient, written row by row through the pool ids by its tail: never C directly
    EXPECT(L.products.dx.dest == GemmDest::Partials || L.products.dx.kernel == GemmKernel::F32Tile64, "%s: dX\n", what);
    product(L.products.dx, "dX", (size_t)-1 / 8, (size_t)-1);
    EXPECT(L.dq_parts == L.products.dq.slices() && L.dq_parts <= kMfmaDqSlices, "%s: dq_parts\n", what);
    EXPECT(room(10) >= (size_t)B * 4, "%s: depth\n", what);
}

// The partial buffer as it was sized before: 8 * B * max(P, De) floats.  Returns whether the plan's scattered product fits it.
static bool old_formula_holds(const Cell &c, const char *no_pair, long long want_written) {
    set_switch("MKB_POOL_NO_MFMA", nullptr); set_switch("MKB_POOL_DENSE", nullptr);
    set_switch("MKB_GEMM_NO128", nullptr); set_switch("MKB_GEMM_BF16X3", nullptr); set_switch("MKB_GEMM_NO_PAIR", no_pair);
    const mkb_tables_t tb = tables(c);
    const int64_t P = 2 * c.K, De = tb.entity_dim;
    PoolPlan L;
    const bool ok = plan_pool(&tb, c.B, P, switches_from_env(), PoolFolds{P <= 1024, true}, L) && L.matrix();
    const long long written = ok ? (long long)L.products.dx.part_floats * 4 : -1, old_room = 8LL * c.B * (P > De ? P : De) * 4;
    printf("hidden %d B %lld K %lld%s: dX writes %lld bytes of partials (ks %d%s); the old formula gave %lld, the plan gives %zu\n", c.d,
           (long long)c.B, (long long)c.K, no_pair ? " MKB_GEMM_NO_PAIR=1" : "", written, ok ? L.products.dx.ks : 0,
           ok && L.products.pair ? ", pair launch" : "", old_room, ok ? L.gemm_part * 4 : (size_t)0);
    EXPECT(written == want_written, "the example's written bytes are %lld, expected %lld\n", written, want_written);
    return written <= old_room;
}

int main() {
    const int models[] = {MKB_TRANSE, MKB_ROTATE, MKB_COMPLEX, MKB_DISTMULT, MKB_PROTATE};
    // the grid of tests/test_host_pool_plan.py ...
    const int dims[] = {3, 30, 64, 100, 255, 256, 257, 500, 512, 513, 1000, 1024, 1025, 1026, 2048, 2049, 2052, 4096, 4097};
    const int64_t batches[] = {1, 7, 60, 256, 1000, 1024, 4096};
    const int64_t sizes[] = {1, 16, 64, 192, 256, 512, 513, 1024, 1025};
    const int relations[] = {11, 237};
    const uintptr_t ents[] = {0x40000000, 0x40000004};
    // ... plus small and odd batches for the two bilinear models (their sizes 192 and 1024 are in the grid already)
    const int64_t more_batches[] = {4, 8, 32, 384};
    const char *no_mfma[] = {nullptr, "1"}, *dense[] = {nullptr, "0", "1"}, *flag[] = {nullptr, "1"}, *bf16x3[] = {nullptr, "0"};

    for (int model : models)
        for (int d : dims) {
            std::vector<int64_t> bs(batches, batches + 7);
            if (model == MKB_COMPLEX || model == MKB_DISTMULT) bs.insert(bs.end(), more_batches, more_batches + 4);
            for (int64_t B : bs)
                for (int64_t K : sizes)
                    for (int n_rel : relations)
                        for (uintptr_t ent : ents) {
                            const Cell c{model, d, B, K, n_rel, ent};
                            const mkb_tables_t tb = tables(c);
                            for (const char *name : {"MKB_POOL_NO_MFMA", "MKB_POOL_DENSE", "MKB_GEMM_NO128", "MKB_GEMM_NO_PAIR", "MKB_GEMM_BF16X3"})
                                unsetenv(name);
                            const int64_t reported = mkb_pool_step_workspace_bytes(&tb, B, K);  // (0: not supported as the environment stands)
                            for (const char *m : no_mfma) for (const char *de : dense) for (const char *n128 : flag) for (const char *np : flag)
                                for (const char *bx : bf16x3) {
                                    set_switch("MKB_POOL_NO_MFMA", m); set_switch("MKB_POOL_DENSE", de);
                                    set_switch("MKB_GEMM_NO128", n128); set_switch("MKB_GEMM_NO_PAIR", np); set_switch("MKB_GEMM_BF16X3", bx);
                                    const PoolSwitches sw = switches_from_env();
                                    PoolPlan L;
                                    if (2 * K > kMaxP) continue;
                                    // mkb_pool_step: the loss rows reduce the scores of pools of <= 1024 positions, the row backward scatters dX
                                    if (plan_pool(&tb, B, 2 * K, sw, PoolFolds{2 * K <= 1024, true}, L) && reported) check_layout(c, L, "step", reported);
                                    if (plan_pool(&tb, B, 2 * K, sw, PoolFolds{false, false}, L) && reported) check_layout(c, L, "score_bwd", reported);
                                }
                        }
        }
    printf("%ld plans, %ld products checked\n", plans, products);

    // the same check on the size the partial buffer had before: it must NOT hold at these shapes
    const bool a = old_formula_holds(Cell{MKB_COMPLEX, 500, 8, 256, 237, 0x40000000}, nullptr, 2048000);
    const bool b = old_formula_holds(Cell{MKB_COMPLEX, 500, 384, 512, 237, 0x40000000}, nullptr, 16384000);
    const bool c = old_formula_holds(Cell{MKB_COMPLEX, 1000, 256, 1024, 237, 0x40000000}, "1", 32768000);
    EXPECT(!a && !b && !c, "the old formula holds at an example where it should not: %d %d %d\n", a, b, c);

    if (failures) { printf("%ld check(s) FAILED\n", failures); return 1; }
    printf("gemm_plan_room_check: ok\n");
    return 0;
}
