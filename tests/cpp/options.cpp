// CPU run of the option and counter tables (cryptonets_amd/csrc/cn_options.h) and the three functions over them, for tests/test_options.py.  No input.  Output:
//     sizeof bytes_of_CnTunables bytes_of_int
//     o name member_index flag lo hi env default_logn13 default_logn14 replan          (env: - = none)
//     c name                                                                            (a counter)
//     e text no_f64 : the 25 members after cn_options_from_env over the defaults of log N = 13, in member order
//                     (every environment name of the table reads `text`, CN_NO_F64 reads `no_f64`; - = not set)
//     s name value : refused value_after          (cn_option_set on a struct that holds `kept`, an allowed value other than the default, in that member)
//     u name : found                               (cn_option_set of a name that is no switch: a counter, a retired switch)
//     g name : found value                         (cn_option_get; the counters hold 1, 2, .. in table order, the last one 2^40)
#include "../../cryptonets_amd/csrc/cn_options.h"
#include <cstdio>
#include <initializer_list>

static int member_index(const CnTunables &t, const OptionSpec &o) { return (int)(((const char *)&(t.*o.member) - (const char *)&t) / sizeof(int)); }

int main() {
    printf("sizeof %zu %zu\n", sizeof(CnTunables), sizeof(int));
    const CnTunables d13 = cn_option_defaults(13), d14 = cn_option_defaults(14);
    for (const OptionSpec &o : kOptions)
        printf("o %s %d %d %d %d %s %d %d %d\n", o.name, member_index(d13, o), (int)o.flag, o.lo, o.hi, o.env ? o.env : "-", d13.*o.member, d14.*o.member, (int)o.replan);
    for (const CounterSpec &c : kCounters) printf("c %s\n", c.name);
    const char *texts[] = {nullptr, "0", "1", "-5", "9"};
    for (const char *text : texts) for (const char *no_f64 : {(const char *)nullptr, "0", "1"}) {
        if (text && !no_f64) continue;
        CnTunables t = d13;
        cn_options_from_env(t, [&](const char *name) { return strcmp(name, "CN_NO_F64") ? text : no_f64; });
        printf("e %s %s :", text ? text : "-", no_f64 ? no_f64 : "-");
        for (size_t i = 0; i < sizeof t / sizeof(int); i++) printf(" %d", ((const int *)&t)[i]);
        printf("\n");
    }
    for (const OptionSpec &o : kOptions) {
        const int def = d13.*o.member, kept = def != o.hi ? o.hi : o.lo;
        for (int value : {o.flag ? 0 : o.lo - 1, o.flag ? 1 : o.lo, o.flag ? 7 : o.hi, o.flag ? -1 : o.hi + 1}) {
            CnTunables t = d13;
            t.*o.member = kept;
            bool refused = false;
            if (cn_option_set(t, o.name, value, &refused) != &o) return 3;
            printf("s %s %d : %d %d\n", o.name, value, (int)refused, t.*o.member);
        }
    }
    CnTunables t = d13;
    CnCounters cnt;
    uint64_t next = 0;
    for (const CounterSpec &c : kCounters) cnt.*c.member = ++next;
    cnt.*kCounters[next - 1].member = 1ull << 40;
    for (const char *name : {"square_gemm_prefloor", "defer", "sq_overlap", "ks_tight", ""}) {
        bool refused = false;
        printf("u %s : %d\n", *name ? name : "-", (int)(cn_option_set(t, name, 1, &refused) != nullptr || refused));
    }
    for (const OptionSpec &o : kOptions) { int v = -99; const bool ok = cn_option_get(t, cnt, o.name, &v); printf("g %s : %d %d\n", o.name, (int)ok, v); }
    for (const CounterSpec &c : kCounters) { int v = -99; const bool ok = cn_option_get(t, cnt, c.name, &v); printf("g %s : %d %d\n", c.name, (int)ok, v); }
    for (const char *name : {"defer", "stream_tries", "defer_stagger"}) { int v = -99; const bool ok = cn_option_get(t, cnt, name, &v); printf("g %s : %d %d\n", name, (int)ok, v); }
    return 0;
}
