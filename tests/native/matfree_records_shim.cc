// C entry points of csrc/matfree_records.h for tests/test_matfree_records_host.py (index functions, plain host code).
#include "../../total-lagrangian-fea_amd/csrc/matfree_records.h"

using namespace tlfea;

extern "C" int mfr_group_of(int real_bytes) { return mfr_group(real_bytes); }
extern "C" long long mfr_len_g(long long E) { return (long long)mfr_g_len((size_t)E); }
extern "C" long long mfr_len_F(long long E, int NP) { return (long long)mfr_F_len((size_t)E, NP); }
// idx [slots][10] with slots = 64 x tiles: position of value t of slot e in the packed g buffer
extern "C" void mfr_fill_g(int G, long long slots, long long* idx) {
  for (long long e = 0; e < slots; e++)
    for (int t = 0; t < kMfrGVals; t++) idx[e * kMfrGVals + t] = (long long)mfr_g_index(G, (size_t)e, t);
}
// idx [slots][NP][9]
extern "C" void mfr_fill_F(int NP, int G, long long slots, long long* idx) {
  for (long long e = 0; e < slots; e++)
    for (int p = 0; p < NP; p++)
      for (int t = 0; t < kMfrFVals; t++) idx[(e * NP + p) * kMfrFVals + t] = (long long)mfr_F_index(NP, G, (size_t)e, p, t);
}
// where the values come from: src10 = position of g value t in the [16] record, slot[NP] = point of the [5][10] record
extern "C" void mfr_sources(int NP, int* src10, int* slot) {
  for (int t = 0; t < kMfrGVals; t++) src10[t] = mfr_g_source(t);
  for (int p = 0; p < NP; p++) slot[p] = mfr_F_slot(NP, p);
}
extern "C" int mfr_group_len_of(int T, int G, int t) { return mfr_group_len(T, G, t); }
