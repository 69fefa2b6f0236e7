// The handle's DH table as a type: the kernels are compiled per table (two static ones, a runtime one per joint count).
// Include behind engine_internal.h and kernels.h.
#pragma once

namespace mt {

template <class Tbl>
struct TableTag {
  using type = Tbl;
};
template <class F>
void with_table(const mt_engine* h, F&& f) {
  if (h->static_kind == 1) return f(TableTag<Ref4Table>{});
  if (h->static_kind == 2) return f(TableTag<Dh7Table>{});
  switch (h->D) {
    case 2: return f(TableTag<RtTable<2>>{});
    case 3: return f(TableTag<RtTable<3>>{});
    case 4: return f(TableTag<RtTable<4>>{});
    case 5: return f(TableTag<RtTable<5>>{});
    case 6: return f(TableTag<RtTable<6>>{});
    case 7: return f(TableTag<RtTable<7>>{});
    case 8: return f(TableTag<RtTable<8>>{});
    default: return;
  }
}

}  // namespace mt
