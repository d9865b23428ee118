// The float rules' kernel launches: every template choice (pack width, mask width, loads in flight, record words, rule,
// degree bucket, first iteration) is made here, from run-time values, each launch written once.  Included by
// run_group.hip.h only: a translation unit that includes this header and calls into Launch<T> instantiates -- compiles --
// T's kernels.
#pragma once
#include "device_decoder_internal.h"

namespace ldpc {

// One per run_group<T> call: the stream and the launch choices that hold for the whole call.  The tunables never affect
// results; `fast` and `corr` carry the implementation's arithmetic.
template <typename T>
struct Launch {
  hipStream_t s;
  bool rec_long;  // some row has more than 8 edges (or "rec_long")
  bool fast;      // "@fast" implementation: the approximate Tanh / Phi rule variants
  // normalized / offset min-sum (Implementation::correction; this one DOES decide results): every min-sum launch below then
  // takes the kernel's corrected instantiation x_kernel<..., dev::MinsumCorr<T>> with c = max(alpha * m - beta, 0) in the
  // decoder's type (kernels_common.hip.h, MinsumCorr) -- there is no plain-arithmetic launch a corrected implementation
  // could fall into
  bool corr;
  dev::MinsumCorr<T> minsum_corr;

  // a min-sum launch, written once: launch(auto... mc) names its kernel with `decltype(mc)...` as the last template arguments
  // and passes `mc...` last -- nothing for plain min-sum, minsum_corr for the corrected forms.  The only reader of `corr`.
  template <typename F>
  auto with_corr(F &&launch) const {
    if (corr) return launch(minsum_corr);
    return launch();
  }
  // a streaming min-sum launch: f(VEC, FIRST, mc...), codewords per lane and first iteration as integral constants
  template <typename F>
  auto minsum(uint32_t vec, bool first, F &&f) const {
    return with_vec<T>(vec, [&](auto V) {
      return with_bool(first, [&](auto FIRST) { return with_corr([&](auto... mc) { return f(V, FIRST, mc...); }); });
    });
  }
  // the rule of an LDS-staged / layered launch: f(RULE, mc...) -- min-sum through with_corr: kRuleMinsumCorr is the
  // kernels' form with mc as the last argument
  template <typename F>
  void with_rule(Rule rule, F &&f) const {
    auto fast_or = [&](auto fast_rule, auto exact_rule) {
      if constexpr (sizeof(T) == 4)
        if (fast) return f(fast_rule);
      f(exact_rule);
    };
    switch (rule) {
      case Rule::Phi: return fast_or(int_c<dev::kRulePhiFast>{}, int_c<dev::kRulePhi>{});
      case Rule::Tanh: return fast_or(int_c<dev::kRuleTanhFast>{}, int_c<dev::kRuleTanh>{});
      case Rule::Minstarapprox: return f(int_c<dev::kRuleMinstarapprox>{});
      case Rule::Aminstar: return f(int_c<dev::kRuleAminstar>{});
      case Rule::Minsum:
        return with_corr([&](auto... mc) { f(int_c<sizeof...(mc) ? dev::kRuleMinsumCorr : dev::kRuleMinsum>{}, mc...); });
    }
  }
  // a launch with dynamic LDS: beyond the 48 KB every kernel may have, the kernel is told first
  template <typename K, typename... A>
  void go(K kernel, const Tiling &t, size_t lds, const A &...args) const {
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds));
    kernel<<<t.blocks, t.threads, lds, s>>>(args...);
  }

  // flooding min-sum check nodes: VEC x mask width x FIRST
  // (eight loads in flight, nontemporal messages: the four-load and the cached-message variants were tuning knobs within
  // a percent of these, gone in round 6)
  void cn_minsum(bool first, uint32_t vec, bool wide_mask, const Tiling &t, const dev::Graph &g, const dev::State &st,
                 const T *L, T *msg, uint32_t *unsat) const {
    minsum(vec, first, [&](auto V, auto FIRST, auto... mc) {
      with_bool(wide_mask, [&](auto wide) {
        using MASK = std::conditional_t<decltype(wide)::value, uint64_t, uint32_t>;
        dev::cn_minsum_kernel<T, decltype(V)::value, MASK, 8, decltype(FIRST)::value, true, decltype(mc)...>
            <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, L, msg, unsat, mc...);
      });
    });
  }
  // L-free variant (double-buffered messages)
  // (four loads in flight, nontemporal stores, cached loads of the previous messages: what round 2 settled on)
  void cn_lfree(bool first, uint32_t vec, bool wide_mask, const Tiling &t, const dev::Graph &g, const dev::State &st,
                const T *chan, T *post, const T *msg_in, T *msg_out, uint32_t *unsat) const {
    minsum(vec, first, [&](auto V, auto FIRST, auto... mc) {
      with_bool(wide_mask, [&](auto wide) {
        using MASK = std::conditional_t<decltype(wide)::value, uint64_t, uint32_t>;
        dev::cn_minsum_lfree_kernel<T, decltype(V)::value, MASK, 4, decltype(FIRST)::value, true, false, decltype(mc)...>
            <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, chan, post, msg_in, msg_out, unsat, mc...);
      });
    });
  }
  // the record form of a flooding launch: f(RECW, F16, F8) -- three words with the flags in the record's own rows, or as
  // 16-bit words in an array of their own (Records::flags), or that array as bytes (Records::flags8: rows of at most 7
  // edges, "flags8"), or four words
  struct Records {
    T *mag;       // the records ([M * recw][tile]); with 16-bit flags the magnitudes alone ([2M][tile])
    void *flags;  // [M][tile] of uint16_t, or null: the flags are the record's third word
    uint32_t recw;
    bool flags8 = false;  // the byte form: `flags` holds [M][tile] of uint8_t (the array keeps its 16-bit size)
  };
  template <typename F>
  static void with_rec_form(const Records &r, F &&f) {
    if (r.recw == 3 && r.flags != nullptr && r.flags8) return f(int_c<3>{}, std::true_type{}, std::true_type{});
    if (r.recw == 3 && r.flags != nullptr) return f(int_c<3>{}, std::true_type{}, std::false_type{});
    if (r.recw == 3) return f(int_c<3>{}, std::false_type{}, std::false_type{});
    f(int_c<4>{}, std::false_type{}, std::false_type{});
  }
  // the records as a kernel argument (dev::RecRef): for a launch that reads them (CONST) or writes them
  template <bool CONST, bool F16, bool F8 = false>
  static auto rec_ref(const Records &r) {
    using TT = std::conditional_t<CONST, const T, T>;
    using FW = dev::RecFlagWord<T, F16, F8>;
    if constexpr (F16)
      return dev::RecPair<TT, FW>{r.mag, static_cast<FW *>(r.flags)};
    else
      return static_cast<TT *>(r.mag);
  }
  // row records (cn_minsum_rec_kernel): VEC x record form x FIRST x long rows
  // (rows of at most 8 edges -- DVB-S2 up to rate 1/2, most 5G NR rows are longer -- take the variant without the
  // further-rounds code)
  // (eight loads in flight per lane; the four-load variant of earlier rounds, a tuning knob nothing selected, is gone)
  // (send = false: no per-edge messages, for a variable-node launch that reads the records -- vn_rec below; 16-bit flags only)
  // (shape: the row-shape form of that kind, "cn_row_shape" -- f32, byte flags, send = false, not the first iteration; the
  // peer table then carries the row-shape counts of that kind, graph_tables.h build_row_shapes.  The caller asks for it only
  // where all of that holds: any other combination is launched in its generic form)
  void cn_rec(bool first, uint32_t vec, const Tiling &t, const dev::Graph &g, const dev::State &st, const T *chan, T *post,
              const Records &in, const Records &out, T *msg, uint32_t *unsat, uint32_t run, bool send = true,
              uint32_t shape = kRowShapeNone) const {
    minsum(vec, first, [&](auto V, auto FIRST, auto... mc) {
      with_rec_form(in, [&](auto W, auto F16, auto F8) {
        with_bool(rec_long, [&](auto long_rows) {
          // (byte flags: rows of at most 7 edges, so only the short-row variant has them; run_group never sets Records::flags8
          // beside rec_long -- every launch of a call must agree on the form)
          constexpr bool kF8 = decltype(F8)::value && !decltype(long_rows)::value;
          // (and so the byte form has seven loads in flight per lane, a whole row, where every other form has eight)
          constexpr int kU = kF8 ? int(kRecFlags8MaxRow) : 8;
          auto go_rec = [&](auto SEND, auto SHAPE) {
            dev::cn_minsum_rec_kernel<T, decltype(V)::value, decltype(W)::value, decltype(F16)::value, kU, decltype(FIRST)::value,
                                      true, false, decltype(long_rows)::value, decltype(SEND)::value, kF8, decltype(SHAPE)::value,
                                      decltype(mc)...>
                <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, chan, post, rec_ref<true, decltype(F16)::value, kF8>(in),
                                                rec_ref<false, decltype(F16)::value, kF8>(out), msg, unsat, run, mc...);
          };
          if constexpr (decltype(F16)::value) {
            if constexpr (kF8 && !decltype(FIRST)::value && sizeof(T) == 4) {
              if (!send && shape == kRowShapePN) return go_rec(std::false_type{}, int_c<dev::kCnShapePN>{});
              if (!send && shape == kRowShapeNP) return go_rec(std::false_type{}, int_c<dev::kCnShapeNP>{});
            }
            if (!send) return go_rec(std::false_type{}, int_c<dev::kCnShapeNone>{});
          }
          go_rec(std::true_type{}, int_c<dev::kCnShapeNone>{});
        });
      });
    });
  }
  void vn_free_rec(uint32_t vec, const Tiling &t, const dev::Graph &g, const dev::State &st, const uint32_t *free_rs,
                   const T *chan, const Records &rec, T *post, int32_t event_iteration) const {
    with_vec<T>(vec, [&](auto V) {
      with_rec_form(rec, [&](auto W, auto F16, auto F8) {
        dev::vn_free_rec_kernel<T, decltype(V)::value, decltype(W)::value, decltype(F16)::value, decltype(F8)::value>
            <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, free_rs, chan, rec_ref<true, decltype(F16)::value, decltype(F8)::value>(rec),
                                            post, event_iteration);
      });
    });
  }
  // the closing launch of a call without a posterior ("call_edges"): the L-free variables' decisions into the packed words
  void vn_free_hard(uint32_t vec, const Tiling &t, const dev::Graph &g, const dev::State &st, const uint32_t *free_rs,
                    const T *chan, const Records &rec, const T *post, uint64_t *bits, uint32_t W) const {
    with_vec<T>(vec, [&](auto V) {
      with_rec_form(rec, [&](auto RW, auto F16, auto F8) {
        dev::vn_free_hard_kernel<T, decltype(V)::value, decltype(RW)::value, decltype(F16)::value, decltype(F8)::value>
            <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, free_rs, chan, rec_ref<true, decltype(F16)::value, decltype(F8)::value>(rec),
                                            post, bits, W);
      });
    });
  }

  // flooding, LDS-staged rules.  reg_dmax: 0 = cn_staged_kernel; 10 / 12 = cn_reg_kernel (rows of at most that many edges
  // in registers; recs: their records).  row_scratch non-null: cn_staged_kernel keeps its columns there (rows beyond the LDS)
  void cn_staged(bool first, Rule rule, uint32_t reg_dmax, const uint32_t *recs, const Tiling &t, size_t lds, T *row_scratch,
                 const dev::Graph &g, const dev::State &st, const T *L, T *msg, uint32_t *unsat, uint32_t dmax) const {
    with_rule(rule, [&](auto rule_c, auto... mc) {
      with_bool(first, [&](auto FIRST) {
        constexpr int RULE = decltype(rule_c)::value;
        // (only the Tanh rule has the register-resident form -- its opt-in "@fast" variant does not; any other rule takes the
        // LDS-staged kernel whatever reg_dmax says: no combination launches nothing)
        if constexpr (RULE == dev::kRuleTanh) {
          if (reg_dmax != 0)
            return with_bool(reg_dmax == 10, [&](auto ten) {
              go(dev::cn_reg_kernel<RULE, T, decltype(ten)::value ? 10 : 12, decltype(FIRST)::value>, t, lds, g, t.sched, st,
                 recs, L, msg, unsat, dmax);
            });
        }
        if (row_scratch)
          go(dev::cn_staged_kernel<RULE, T, decltype(FIRST)::value, true, decltype(mc)...>, t, 0, g, t.sched, st, L, msg,
             unsat, dmax, row_scratch, mc...);
        else
          go(dev::cn_staged_kernel<RULE, T, decltype(FIRST)::value, false, decltype(mc)...>, t, lds, g, t.sched, st, L, msg,
             unsat, dmax, nullptr, mc...);
      });
    });
  }

  // variable nodes: every form is a launch of dev::vn_kernel, written here once.  src...: what it sums, the kernel's SRC
  // arguments (the per-edge messages, or the records and keep_rs).  EVW, EVF16, EVF8: the record form of ev_rec, the event
  // block's records (null, or EVW == 0: no event block)
  // (eight loads in flight)
  template <int VEC, bool NT, bool LIST, int EVW, bool EVF16, bool EVF8, typename... SRC>
  void vn_go(const Tiling &t, const dev::Graph &g, const dev::State &st, const T *chan, T *post, const uint32_t *unsat_in,
             uint32_t *unsat_clear, int32_t latch_it, const uint32_t *free_var, const uint32_t *free_rs, const Records *ev_rec,
             uint32_t n_free, SRC... src) const {
    dev::VnEventOf<T, EVF16, EVF8> ev{};
    if (ev_rec) ev = dev::VnEventOf<T, EVF16, EVF8>{free_var, free_rs, rec_ref<true, EVF16, EVF8>(*ev_rec), n_free};
    dev::vn_kernel<T, VEC, 8, NT, LIST, EVW, EVF16, EVF8, SRC...>
        <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, chan, src..., post, unsat_in, unsat_clear, latch_it, ev);
  }
  typedef const T *__restrict__ MsgIn;  // (SRC as the kernels have always declared these arguments)
  typedef const uint32_t *__restrict__ TableIn;
  // from the per-edge messages (list = true: only the variables of Graph::list_*)
  // (the messages are read once: nontemporal -- 732 -> 680 us on DVB-S2 1/2 in round 2)
  void vn(bool list, uint32_t vec, const Tiling &t, const dev::Graph &g, const dev::State &st, const T *chan, const T *msg,
          T *post, const uint32_t *unsat_in, uint32_t *unsat_clear, int32_t latch_it) const {
    with_vec<T>(vec, [&](auto V) {
      with_bool(list, [&](auto LIST) {
        vn_go<decltype(V)::value, true, decltype(LIST)::value, 0, false, false, MsgIn>(
            t, g, st, chan, post, unsat_in, unsat_clear, latch_it, nullptr, nullptr, nullptr, 0, msg);
      });
    });
  }
  // the list variant that also rebuilds the L-free posteriors of a slice's first convergences (kernels_flooding.hip.h, EVW)
  // (free_var, free_rs, n_free: the L-free variables; rec: the records of the iteration being latched)
  void vn_event(uint32_t vec, const Tiling &t, const dev::Graph &g, const dev::State &st, const T *chan, const T *msg, T *post,
                const uint32_t *unsat_in, uint32_t *unsat_clear, int32_t latch_it, const uint32_t *free_var,
                const uint32_t *free_rs, const Records &rec, uint32_t n_free) const {
    with_vec<T>(vec, [&](auto V) {
      with_rec_form(rec, [&](auto W, auto F16, auto F8) {
        vn_go<decltype(V)::value, true, true, decltype(W)::value, decltype(F16)::value, decltype(F8)::value, MsgIn>(
            t, g, st, chan, post, unsat_in, unsat_clear, latch_it, free_var, free_rs, &rec, n_free, msg);
      });
    });
  }

  // the list variant that sums the kept variables from the records of this iteration (kernels_flooding.hip.h, REC; 16-bit
  // flags, or the same records with byte flags).  ev_rec null: no event block (the first iteration, or "vn_event" /
  // "rec_quiet" off).
  // (eight records in flight and nontemporal channel loads: the headline gains 0.65 % over four in flight -- 98 against 57
  // VGPRs, 4 against 8 waves per SIMD -- and 0.35 % over cached channel loads, profiles/vn_records.txt section 1)
  // chain non-null: g's list and keep_rs are the chained ones (graph_tables.h, build_vn_chains) and t is chain_tiling's
  void vn_rec(uint32_t vec, const Tiling &t, const dev::Graph &g, const dev::State &st, const T *chan,
              const Records &rec, const uint32_t *keep_rs, T *post, const uint32_t *unsat_in, uint32_t *unsat_clear,
              int32_t latch_it, const uint32_t *free_var, const uint32_t *free_rs, const Records *ev_rec, uint32_t n_free,
              const dev::VnChain *chain = nullptr) const {
    with_vec<T>(vec, [&](auto V) {
      with_bool(ev_rec != nullptr, [&](auto EV) {
        with_bool(rec.flags8, [&](auto F8) {
          constexpr bool kF8 = decltype(F8)::value;
          using RecIn = typename dev::RecRef<T, true, kF8>::in;
          if (chain)
            return vn_go<decltype(V)::value, true, true, decltype(EV)::value ? 3 : 0, true, kF8, RecIn, TableIn, dev::VnChain>(
                t, g, st, chan, post, unsat_in, unsat_clear, latch_it, free_var, free_rs, ev_rec, n_free,
                rec_ref<true, true, kF8>(rec), keep_rs, *chain);
          vn_go<decltype(V)::value, true, true, decltype(EV)::value ? 3 : 0, true, kF8, RecIn, TableIn>(
              t, g, st, chan, post, unsat_in, unsat_clear, latch_it, free_var, free_rs, ev_rec, n_free,
              rec_ref<true, true, kF8>(rec), keep_rs);
        });
      });
    });
  }
  // The chained launch's waves follow from the blocks: a slice's waves come in groups of `mates` -- the waves of a workgroup
  // that see the same codewords, where the slice's waves divide into such groups, else 1 -- and a group walks whole blocks,
  // so no more groups than blocks.  Fills chain->mates and chain->n_groups (len, width, n_blocks: the tables').
  static Tiling chain_tiling(uint32_t G, uint32_t tile, uint32_t slice, uint32_t threads, uint32_t target_waves,
                             dev::VnChain *chain) {
    const uint32_t wpb = threads / 64, spt = std::max<uint32_t>(1, tile / slice);
    uint32_t mates = (spt <= wpb && wpb % spt == 0) ? wpb / spt : 1;
    mates = std::min(mates, chain->width);
    if (chain->width % mates != 0) mates = 1;
    Tiling t = make_tiling(G, tile, slice, std::max<uint32_t>(chain->n_blocks, 1) * mates, threads, target_waves);
    if (t.sched.waves_per_chunk % mates != 0) mates = 1;
    chain->mates = mates;
    chain->n_groups = t.sched.waves_per_chunk / mates;
    return t;
  }

  // layered
  // reg_dmax: 0 = two-pass kernel (row_scratch non-null: its columns there); 10 / 12 / 24 = register-resident rows of at
  // most that many edges
  void hl(bool first, Rule rule, uint32_t reg_dmax, const Tiling &t, size_t lds, T *row_scratch, const dev::Graph &g,
          const dev::State &st, const uint32_t *level_rows, uint32_t n_level, T *Q, T *R, uint32_t dmax) const {
    with_rule(rule, [&](auto rule_c, auto... mc) {
      with_bool(first, [&](auto FIRST) {
        constexpr int RULE = decltype(rule_c)::value;
        auto reg = [&](auto DMAX) {
          go(dev::hl_level_reg_kernel<RULE, T, decltype(DMAX)::value, decltype(FIRST)::value, decltype(mc)...>, t, lds, g,
             t.sched, st, level_rows, n_level, Q, R, dmax, mc...);
        };
        if (reg_dmax == 10)
          reg(int_c<10>{});
        else if (reg_dmax == 12)
          reg(int_c<12>{});
        else if (reg_dmax == 24)
          reg(int_c<24>{});
        else if (row_scratch)
          go(dev::hl_level_kernel<RULE, T, decltype(FIRST)::value, true, decltype(mc)...>, t, 0, g, t.sched, st, level_rows,
             n_level, Q, R, dmax, row_scratch, mc...);
        else
          go(dev::hl_level_kernel<RULE, T, decltype(FIRST)::value, false, decltype(mc)...>, t, lds, g, t.sched, st,
             level_rows, n_level, Q, R, dmax, nullptr, mc...);
      });
    });
  }

  // layered min-sum, streaming
  void hl_minsum(bool first, uint32_t vec, const Tiling &t, const dev::Graph &g, const dev::State &st,
                 const uint32_t *level_rows, uint32_t n_level, T *Q, T *R) const {
    minsum(vec, first, [&](auto V, auto FIRST, auto... mc) {
      dev::hl_minsum_kernel<T, decltype(V)::value, 8, decltype(FIRST)::value, decltype(mc)...>
          <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, level_rows, n_level, Q, R, mc...);
    });
  }
  // register-resident rows: DMAX bucket of the level's largest row; vec capped so that the
  // 2 * DMAX * VEC values fit the register file with some occupancy left
  // 0 = no register-resident form for this level (rows too long for the register budget even with
  // one codeword per lane: the two-pass kernel takes it)
  static uint32_t hl_reg_bucket(uint32_t maxdeg) {
    const uint32_t dmax = maxdeg <= 8 ? 8 : (maxdeg <= 12 ? 12 : (maxdeg <= 20 ? 20 : (maxdeg <= 32 ? 32 : 0)));
    return 2 * dmax * (sizeof(T) / 4) <= 96 ? dmax : 0;
  }
  static uint32_t hl_reg_vec(uint32_t vec, uint32_t dmax) {
    const uint32_t words = sizeof(T) / 4;
    while (vec > 1 && 2 * dmax * vec * words > 96) vec /= 2;
    return vec;
  }
  // a bucket of hl_reg_bucket as a template argument; false: there is no such bucket
  template <typename F>
  static bool with_bucket(uint32_t dmax, F &&f) {
    switch (dmax) {
      case 8: return f(int_c<8>{});
      case 12: return f(int_c<12>{});
      case 20: return f(int_c<20>{});
      case 32: return f(int_c<32>{});
      default: return false;
    }
  }
  // returns false when the (VEC, DMAX) pair has no instantiation (the caller must not let that pass): the 20-edge bucket
  // exists with VEC * sizeof(T) <= 8, the 32-edge one with <= 4
  bool hl_minsum_reg(bool first, uint32_t vec, uint32_t dmax, const Tiling &t, const dev::Graph &g, const dev::State &st,
                     const uint32_t *level_rows, uint32_t n_level, T *Q, T *R) const {
    return minsum(vec, first, [&](auto V, auto FIRST, auto... mc) {
      return with_bucket(dmax, [&](auto D) {
        constexpr int VEC = decltype(V)::value, DMAX = decltype(D)::value;
        if constexpr (DMAX <= 12 || VEC * sizeof(T) <= (DMAX == 20 ? 8u : 4u)) {
          dev::hl_minsum_reg_kernel<T, VEC, DMAX, decltype(FIRST)::value, decltype(mc)...>
              <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, level_rows, n_level, Q, R, mc...);
          return true;
        } else {
          return false;
        }
      });
    });
  }
  // layered min-sum with row records (hl_minsum_rec_kernel; three-word records only): the row's Qv values and two
  // records live in registers
  static uint32_t hl_rec_vec(uint32_t vec, uint32_t dmax) {
    const uint32_t words = sizeof(T) / 4;
    while (vec > 1 && (dmax + 6) * vec * words > 112) vec /= 2;
    return vec;
  }
  // (false as above: a pair beyond hl_rec_vec's register budget has no instantiation)
  bool hl_minsum_rec(bool first, uint32_t vec, uint32_t dmax, const Tiling &t, const dev::Graph &g, const dev::State &st,
                     const uint32_t *level_rows, uint32_t n_level, T *Q, T *rec) const {
    return minsum(vec, first, [&](auto V, auto FIRST, auto... mc) {
      return with_bucket(dmax, [&](auto D) {
        constexpr int VEC = decltype(V)::value, DMAX = decltype(D)::value;
        constexpr uint32_t kWords = VEC * sizeof(T) / 4;
        if constexpr (DMAX <= 12 || (DMAX + 6) * kWords <= 112) {
          dev::hl_minsum_rec_kernel<T, VEC, DMAX, 3, decltype(FIRST)::value, decltype(mc)...>
              <<<t.blocks, t.threads, 0, s>>>(g, t.sched, st, level_rows, n_level, Q, rec, mc...);
          return true;
        } else {
          return false;
        }
      });
    });
  }
};

}  // namespace ldpc
