// The host side of csrc/yk_optarg.h as plain C++17 (tests/test_optarg_host.py builds and runs this): prints what
// with_opts hands its callback for every on/off setting of three options, and what opt_arg, get_arg and args_in
// give; the test holds the lines against its own table.
#include <cstdio>
#include <string>
#include <type_traits>

#include "yk_optarg.h"

struct A { int x; };
struct B1 { int x; };
struct B2 { int x; };  // option B carries two values, (B1, B2)
struct C { int x; };

template <class T>
const char* name() {
    static_assert(!std::is_reference_v<T> && !std::is_const_v<T>, "the decayed type");
    if (std::is_same_v<T, A>) return "A";
    if (std::is_same_v<T, B1>) return "B1";
    if (std::is_same_v<T, B2>) return "B2";
    if (std::is_same_v<T, C>) return "C";
    return "?";
}

// the order / uniqueness check, as constants
constexpr bool OK_NONE = yk::args_in(yk::Args<A, C>{}, yk::Args<>{});
constexpr bool OK_A = yk::args_in(yk::Args<A, C>{}, yk::Args<A>{});
constexpr bool OK_C = yk::args_in(yk::Args<A, C>{}, yk::Args<C>{});
constexpr bool OK_AC = yk::args_in(yk::Args<A, C>{}, yk::Args<A, C>{});
constexpr bool OK_CA = yk::args_in(yk::Args<A, C>{}, yk::Args<C, A>{});
constexpr bool OK_AA = yk::args_in(yk::Args<A, C>{}, yk::Args<A, A>{});
constexpr bool OK_B = yk::args_in(yk::Args<A, C>{}, yk::Args<B1>{});  // a type the list does not have
static_assert(yk::has_arg<C, A, C> && !yk::has_arg<B1, A, C> && !yk::has_arg<A>, "has_arg");

int main() {
    for (int m = 0; m < 8; m++) {
        const bool a = m & 4, b = m & 2, c = m & 1;
        int calls = 0;
        std::string types, values;
        yk::with_opts(
            [&](const auto&... o) {
                calls++;
                ((types += std::string(name<std::decay_t<decltype(o)>>()) + ","), ...);
                ((values += std::to_string(o.x) + ","), ...);
            },
            yk::opt(a, A{10 + m}), yk::opt(b, B1{20 + m}, B2{30 + m}), yk::opt(c, C{40 + m}));
        std::printf("with_opts %d%d%d calls=%d types=%s values=%s\n", a, b, c, calls, types.c_str(), values.c_str());
    }
    const A a{1};
    const C c{3};
    std::printf("opt_arg present=%d first=%d absent=%d empty=%d\n", yk::opt_arg(C{-1}, a, c).x, yk::opt_arg(A{-1}, a, c).x,
                yk::opt_arg(B1{-1}, a, c).x, yk::opt_arg(B1{-2}).x);
    std::printf("get_arg same=%d %d\n", &yk::get_arg<C>(a, c) == &c, &yk::get_arg<A>(a, c) == &a);
    std::printf("args_in ()=%d (A)=%d (C)=%d (A,C)=%d (C,A)=%d (A,A)=%d (B1)=%d\n", OK_NONE, OK_A, OK_C, OK_AC, OK_CA, OK_AA,
                OK_B);
    return 0;
}
