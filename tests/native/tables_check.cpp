// Stand-alone run of the host table builder (csrc/pd_tables.hip), meant for host sanitizers: built
// together with pd_tables.hip, no GPU and no libpdenv.so.  argv[1]: the image of a pd_params
// followed by its keys_cd and keys_cl arrays (tests/test_tables_sanitized.py writes it); the
// pointers are re-based here and the ascent reference trajectory's are nulled.  Builds the default
// tables of a binary64 and a binary32 handle, checks that every recorded slot names the hash entry
// of its recorded key, and prints "ok" and an FNV-1a digest of every array of HostTables (the
// digests are the same for any build with the product's floating point flags).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pd_tables.h"

using namespace pd;

namespace pd {
pd_status set_error(pd_status s, const char* m) { std::fprintf(stderr, "tables_check: %s\n", m); return s; }
}  // namespace pd

namespace {

long bad = 0;
void expect(bool ok, const char* what, const char* tag, long i) {
    if (!ok && ++bad <= 20) std::fprintf(stderr, "tables_check: %s: %s at %ld\n", tag, what, i);
}

uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t*)p)[i]; h *= 1099511628211ull; }
    return h;
}
template <typename T> void digest(const char* tag, const char* name, const std::vector<T>& v) {
    std::printf("%s %-16s %9zu %016llx\n", tag, name, v.size(), (unsigned long long)fnv(v.data(), v.size() * sizeof(T)));
}

// slot (flags stripped by the caller) is an occupied entry of T holding key
template <typename R> bool names(const Table<R>& T, int slot, unsigned long long key) {
    return slot >= 0 && (size_t)slot < T.keys.size() && T.keys[slot] != kEmptyKey && T.keys[slot] == key;
}

template <typename R> void check(const char* tag, const pd_params& p) {
    pd_config c{};
    c.n_envs = 1; c.phase = PD_PHASE_PURE_THROTTLE; c.rtd = PD_RTD_RL;
    c.precision = sizeof(R) == 8 ? PD_F64 : PD_F32;
    c.discount_factor = 0.99; c.trajectory_length = 100;
    HostTables<R>* Hp = new HostTables<R>();
    HostTables<R>& H = *Hp;
    if (build_host_tables<R>(&p, &c, H) != PD_OK) { ++bad; delete Hp; return; }
    const Table<R>* T[2] = {&H.cd, &H.cl};
    const int lowmask = kGridPiece - 1;
    for (int tb = 0; tb < 2; ++tb) {
        int64_t occ = 0;
        for (unsigned long long k : T[tb]->keys) occ += k != kEmptyKey;
        expect(occ == T[tb]->entries, "entries differs from the occupied hash entries", tag, tb);
        const auto& G = H.grid[tb];
        const int S2 = kGridSub * kGridSub;
        expect(G.key.size() == (size_t)G.nm * G.na && G.slot.size() == G.key.size(), "grid size", tag, tb);
        expect(G.sub_key.size() == G.sub_slot.size() && G.sub_key.size() % S2 == 0, "sub-grid size", tag, tb);
        for (size_t i = 0; i < G.slot.size(); ++i) {
            const int s = G.slot[i];
            if (s < 0) continue;
            if (s & kGridRefine) expect((size_t)(s & (kGridRefine - 1)) < G.sub_key.size() / S2, "refined index out of range", tag, (long)i);
            else expect(names(*T[tb], s & lowmask, G.key[i]), "grid slot does not name its key", tag, (long)i);
        }
        for (size_t i = 0; i < G.sub_slot.size(); ++i) {
            const int s = G.sub_slot[i];
            if (s < 0) continue;
            if (s & kGridBisect) expect((size_t)(s & (kGridBisect - 1)) < G.bis.size(), "bisector index out of range", tag, (long)i);
            else expect(names(*T[tb], s & lowmask, G.sub_key[i]), "sub-cell slot does not name its key", tag, (long)i);
        }
        for (size_t i = 0; i < G.bis.size(); ++i) {
            const GridBisect& b = G.bis[i];
            if (b.slot_a >= 0) expect(names(*T[tb], b.slot_a & lowmask, b.key_a), "bisector slot_a does not name key_a", tag, (long)i);
            if (b.slot_b >= 0) expect(names(*T[tb], b.slot_b & lowmask, b.key_b), "bisector slot_b does not name key_b", tag, (long)i);
        }
    }
    for (int li = 0; li < 4; ++li)
        for (int k = 0; k <= H.D.line_nbp[li]; ++k)
            if (H.D.line_slot[li][k] >= 0)
                expect(names(*T[li / 2], H.D.line_slot[li][k], H.D.line_key[li][k]), "line slot does not name its key", tag, li * 1000 + k);
    std::printf("%s %-16s %9zu %016llx\n", tag, "params", sizeof(H.D), (unsigned long long)fnv(&H.D, sizeof(H.D)));
    digest(tag, "atm", H.atm);
    digest(tag, "tay", H.tay);
    for (int tb = 0; tb < 2; ++tb) {
        const std::string n = tb ? "cl." : "cd.";
        const auto& G = H.grid[tb];
        std::printf("%s %-16s %9lld %9d\n", tag, (n + "entries").c_str(), (long long)T[tb]->entries, T[tb]->logcap);
        digest(tag, (n + "keys").c_str(), T[tb]->keys);
        digest(tag, (n + "pay").c_str(), T[tb]->pay);
        digest(tag, (n + "grid_key").c_str(), G.key);
        digest(tag, (n + "grid_slot").c_str(), G.slot);
        digest(tag, (n + "sub_key").c_str(), G.sub_key);
        digest(tag, (n + "sub_slot").c_str(), G.sub_slot);
        digest(tag, (n + "bis").c_str(), G.bis);
        if (!G.pieces) continue;
        const bool f32 = sizeof(R) == 4;
        if (f32) digest(tag, (n + "cell_rec").c_str(), G.pieces->rec32); else digest(tag, (n + "cell_rec").c_str(), G.pieces->rec);
        digest(tag, (n + "cell_sub").c_str(), f32 ? G.pieces->sub_piece32 : G.pieces->sub_piece);
        digest(tag, (n + "cell_fine").c_str(), f32 ? G.pieces->fine32 : G.pieces->fine);
    }
    delete Hp;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: tables_check params.bin\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<uint8_t> img;
    uint8_t buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) img.insert(img.end(), buf, buf + n);
    std::fclose(f);
    pd_params P;
    if (img.size() < sizeof(P)) { std::fprintf(stderr, "tables_check: image shorter than pd_params\n"); return 2; }
    std::memcpy(&P, img.data(), sizeof(P));
    if (P.n_keys_cd < 0 || P.n_keys_cl < 0 || img.size() != sizeof(P) + 8 * (size_t)(P.n_keys_cd + P.n_keys_cl)) {
        std::fprintf(stderr, "tables_check: image size does not match the key counts\n");
        return 2;
    }
    std::vector<uint64_t> keys((size_t)(P.n_keys_cd + P.n_keys_cl));
    std::memcpy(keys.data(), img.data() + sizeof(P), keys.size() * 8);
    P.keys_cd = keys.data(); P.keys_cl = keys.data() + P.n_keys_cd;
    P.ref_y = P.ref_x = P.ref_vx = P.ref_vy = nullptr;
    check<double>("f64", P);
    check<float>("f32", P);
    if (bad) { std::fprintf(stderr, "tables_check: %ld failed checks\n", bad); return 1; }
    std::printf("ok\n");
    return 0;
}
