// Stand-alone driver of dfmdock_amd/csrc/dfm_schedule.h for tests/test_schedule_cpu.py (built by g++ with the address and
// undefined-behaviour sanitizers; no HIP, no library).
//   schedule_main grid T_FIRST EPS NUM_STEPS FLAGS TR_NOISE ROT_NOISE R3_MIN R3_MAX SO3_MIN SO3_MAX
//       rc, then ts / dt / g / sigma as hex doubles and every StepParams field of every step as bits
//   schedule_main sel                  EngineSel (and table_by_default) of the 16 combinations of the four engine flags
//   schedule_main key B FLAGS L0 RESTR [B FLAGS L0 RESTR ...]      graph_key of each
//   schedule_main finite N [OFFSET:HEXWORD ...]      first_nonfinite of N finite floats with the listed words planted
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dfm_schedule.h"

static uint32_t bits(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}

static int grid(char **a)
{
    dfm_hparams hp;
    std::memset(&hp, 0, sizeof(hp));
    const float t_first = strtof(a[0], nullptr), eps = strtof(a[1], nullptr);
    const int n = atoi(a[2]);
    const uint32_t flags = (uint32_t)strtoul(a[3], nullptr, 0);
    const float trn = strtof(a[4], nullptr), rotn = strtof(a[5], nullptr);
    hp.r3_min_sigma = strtod(a[6], nullptr); hp.r3_max_sigma = strtod(a[7], nullptr);
    hp.so3_min_sigma = strtod(a[8], nullptr); hp.so3_max_sigma = strtod(a[9], nullptr);
    dfm::TimeGrid g;
    const int rc = dfm::time_grid(hp, t_first, eps, n, &g);
    printf("rc %d\n", rc);
    if (rc) return 0;
    printf("dt %a\n", (double)g.dt);
    printf("ts");
    for (int i = 0; i < n; ++i) printf(" %a", (double)g.ts[i]);
    printf("\ngr");
    for (int i = 0; i < n; ++i) printf(" %a", g.gr[i]);
    printf("\ngt");
    for (int i = 0; i < n; ++i) printf(" %a", g.gt[i]);
    for (int which = 0; which < 2; ++which) {      // sigma, and g again through the public shape of the call
        printf("\nsigma%d", which);
        for (int i = 0; i < n; ++i) {
            double gg = 0, s = 0;
            if (dfm::diffusion_coef(hp, which, (double)g.ts[i], &gg, &s) != DFM_OK || gg != (which ? g.gr[i] : g.gt[i])) return 3;
            printf(" %a", s);
        }
    }
    std::vector<dfm::StepParams> sp(n);
    for (int i = 0; i < n; ++i) sp[i] = dfm::step_params(g, i, flags, trn, rotn, n);
    const char *names[10] = {"g2_r", "g_r", "hg2_r", "g2_t", "g_t", "hg2_t", "dt_f", "sqrt_dt", "rot_noise", "tr_noise"};
    for (int k = 0; k < 10; ++k) {
        printf("\n%s", names[k]);
        for (int i = 0; i < n; ++i) {
            const dfm::StepParams &p = sp[i];
            const float v[10] = {p.g2_r, p.g_r, p.hg2_r, p.g2_t, p.g_t, p.hg2_t, p.dt, p.sqrt_dt, p.rot_noise, p.tr_noise};
            printf(" %u", bits(v[k]));
        }
    }
    printf("\nstep");
    for (int i = 0; i < n; ++i) printf(" %u", sp[i].step);
    printf("\npad");
    for (int i = 0; i < n; ++i) printf(" %u", sp[i].pad);
    printf("\nsizeof %zu\n", sizeof(dfm::StepParams));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 12 && !strcmp(argv[1], "grid")) return grid(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "sel")) {
        for (int c = 0; c < 16; ++c) {
            const uint32_t flags = (c & 1 ? DFM_F_MFMA16 : 0u) | (c & 2 ? DFM_F_F16 : 0u) | (c & 4 ? DFM_F_BF16_OPS : 0u) | (c & 8 ? DFM_F_NO_L0_TABLE : 0u);
            const dfm::EngineSel s = dfm::engine_sel(flags);
            printf("%u %d %d %d %d %d\n", flags, (int)s.bf16, (int)s.f16, (int)s.bf16_ops, (int)s.has_table, (int)dfm::table_by_default(s, flags));
        }
        return 0;
    }
    if (argc >= 6 && (argc - 2) % 4 == 0 && !strcmp(argv[1], "key")) {
        for (int k = 2; k < argc; k += 4)
            printf("%llu\n", (unsigned long long)dfm::graph_key(atoi(argv[k]), (uint32_t)strtoul(argv[k + 1], nullptr, 0), atoi(argv[k + 2]) != 0,
                                                               atoi(argv[k + 3]) != 0));
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "finite")) {      // its own heap block of exactly N floats: a scan past it is a sanitizer report
        const size_t n = (size_t)strtoull(argv[2], nullptr, 10);
        float *x = n ? static_cast<float *>(malloc(n * sizeof(float))) : nullptr;
        if (n && !x) return 3;
        for (size_t k = 0; k < n; ++k) x[k] = 1.0f + (float)(k % 7);
        for (int a = 3; a < argc; ++a) {
            unsigned long long off = 0; unsigned int word = 0;
            if (sscanf(argv[a], "%llu:%x", &off, &word) != 2 || off >= n) { free(x); return 2; }
            std::memcpy(x + off, &word, 4);
        }
        printf("%zu\n", dfm::first_nonfinite(x, n));
        free(x);
        return 0;
    }
    fprintf(stderr, "usage: %s grid ... | sel | key ... | finite N [OFFSET:HEXWORD ...]\n", argv[0]);
    return 2;
}
