// yk_optarg.h - optional kernel arguments, picked by type.  An opt-in feature's parameters
// travel in its own kernel argument, which exists only in the instantiations that read it: the kernel takes a
// pack after its fixed arguments, a type in the pack switches the feature on, and the default instantiation -
// the empty pack - keeps the arguments, and with them the code, it had without the feature (one more argument,
// even unread, changes the register allocation).  Adding an option to a kernel: one type in its args_in list,
// one opt(...) in each of its launches.  Plain C++17 as well as HIP (tests/optarg_host.cpp).
#pragma once
#include <tuple>
#include <type_traits>

#ifndef __HIPCC__
#define __host__
#define __device__
#define __forceinline__
#endif

namespace yk {

// whether the pack A... has a T
template <class T, class... A>
inline constexpr bool has_arg = (std::is_same_v<T, A> || ...);

// the pack's T, or dflt when the pack has none: for a value that is forwarded either way
template <class T>
__host__ __device__ __forceinline__ T opt_arg(const T& dflt) { return dflt; }
template <class T, class A0, class... A>
__host__ __device__ __forceinline__ T opt_arg(const T& dflt, const A0& a0, const A&... a) {
    if constexpr (std::is_same_v<T, A0>) return a0;
    else return opt_arg(dflt, a...);
}
// the pack's T itself; the pack has one (under if constexpr (has_arg<T, A...>))
template <class T, class A0, class... A>
__host__ __device__ __forceinline__ const T& get_arg(const A0& a0, const A&... a) {
    if constexpr (std::is_same_v<T, A0>) return a0;
    else return get_arg<T>(a...);
}

// whether the pack A... holds only types of the list L..., each at most once, in the list's order: a kernel's
// static_assert, so that an instantiation has one spelling and one argument layout
template <class... T>
struct Args {};
template <class... L>
constexpr bool args_in(Args<L...>, Args<>) { return true; }
template <class A0, class... A>
constexpr bool args_in(Args<>, Args<A0, A...>) { return false; }
template <class L0, class... L, class A0, class... A>
constexpr bool args_in(Args<L0, L...>, Args<A0, A...>) {
    if constexpr (std::is_same_v<L0, A0>) return args_in(Args<L...>{}, Args<A...>{});
    else return args_in(Args<L...>{}, Args<A0, A...>{});
}

// The launch (host).  opt: an option - whether it is on, and the value, or the values, each its own kernel
// argument, that it adds.  with_opts: f(v...) once, v the values of the options that are on, in the order given;
// f is generic and names the kernel's pack by the values' types, k<std::decay_t<decltype(o)>...>.
template <class... T>
struct Opt {
    bool on;
    std::tuple<T...> v;
};
template <class... T>
Opt<T...> opt(bool on, const T&... v) { return Opt<T...>{on, std::tuple<T...>(v...)}; }
template <class F>
void with_opts(F&& f) { f(); }
template <class F, class... T, class... R>
void with_opts(F&& f, const Opt<T...>& o, const R&... r) {
    if (o.on) with_opts([&](const auto&... a) { std::apply([&](const T&... v) { f(v..., a...); }, o.v); }, r...);
    else with_opts(f, r...);
}

}  // namespace yk
