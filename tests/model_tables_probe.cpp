// model_tables_probe.cpp — csrc/model_tables.h behind two C functions, for
// tests/test_model_tables.py: built with the host compiler into a shared object (no HIP
// runtime, no GPU) and loaded with ctypes.
#include <cstring>
#include <map>

#include "model_tables.h"

namespace {
mjx::ModelTables g_tables;
std::string g_err;

template <class T>
std::pair<const void*, size_t> span(const std::vector<T>& v) { return {v.data(), v.size() * sizeof(T)}; }
}  // namespace

extern "C" {

// Runs build_model_tables; returns "" or the refusal.  The tables stay until the next call.
const char* mt_build(const mjxModelDesc* desc) {
  g_tables = mjx::ModelTables();
  g_err = mjx::build_model_tables(*desc, g_tables);
  return g_err.c_str();
}

// Copies the named table of the last build to `out` (at most `cap` bytes); returns its size
// in bytes, or -1 for an unknown name.  "dims" is engine.h Dims as ints, "scalars" is
// {nmaskword, ncsens}.
long mt_table(const char* name, void* out, long cap) {
  const mjx::ModelTables& t = g_tables;
  const int scalars[2] = {t.nmaskword, t.ncsens};
  const std::map<std::string, std::pair<const void*, size_t>> all = {
      {"dims", {&t.d, sizeof(t.d)}}, {"scalars", {scalars, sizeof(scalars)}},
      {"dof_parentid", span(t.dof_parentid)}, {"dof_ancmask", span(t.dof_ancmask)},
      {"body_submask", span(t.body_submask)}, {"body_dofmask", span(t.body_dofmask)},
      {"body_rec", span(t.body_rec)}, {"dof_rec", span(t.dof_rec)}, {"act_rec", span(t.act_rec)},
      {"geom_lds", span(t.geom_lds)}, {"lds_geom", span(t.lds_geom)}, {"st_geom", span(t.st_geom)},
      {"st_pairadr", span(t.st_pairadr)}, {"st_partner", span(t.st_partner)},
      {"st_aabb", span(t.st_aabb)}, {"st_chunk_aabb", span(t.st_chunk_aabb)},
      {"pair_rec", span(t.pair_rec)}, {"cs_sensor", span(t.cs_sensor)},
      {"geom_csmask1", span(t.geom_csmask1)}, {"geom_csmask2", span(t.geom_csmask2)},
      {"static_geoms", span(t.static_geoms)}, {"static_xpos", span(t.static_xpos)},
      {"static_xmat", span(t.static_xmat)}, {"sensor_ext", span(t.sensor_ext)}};
  const auto it = all.find(name);
  if (it == all.end()) return -1;
  const long n = (long)it->second.second;
  if (out && n > 0) std::memcpy(out, it->second.first, (size_t)(n < cap ? n : cap));
  return n;
}

}  // extern "C"
