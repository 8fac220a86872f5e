// jit.hip — the step kernels specialised for ONE model at run time (mjlab_amd/jit.py): the
// same kernel source as spec.hip, compiled by hipcc when a Simulation's model matches no
// csrc/specs.inc entry, into a small shared library that libmjx355 loads and registers
// (mjx_spec_register).  Set by the build: MJX_SPECS_FILE (a generated specs file holding the
// entry) and MJX_JIT_ID (its id: distinct per entry, so that no template instantiation
// shares a name with the main library's or another JIT library's; built with
// -fvisibility=hidden, only the two entry points below are exported).
#include "engine_impl.h"

#ifndef MJX_JIT_ID
#error "MJX_JIT_ID must name the generated entry"
#endif

namespace mjx {
static_assert(Spec<MJX_JIT_ID>::on, "the generated specs file lacks the entry");
}  // namespace mjx

#ifndef MJX_HDR_HASH
#error "MJX_HDR_HASH must be the kernel-header hash (mjlab_amd/jit.py, csrc/Makefile)"
#endif
// engine.h JitInfo: the struct size (the caller's must equal it), the kernel headers this
// library was compiled from (must equal libmjx355's own) and the key that selects its kernels
extern "C" __attribute__((visibility("default"))) void mjx_jit_describe(mjx::JitInfo* out) {
  const bool same = out->size == (int)sizeof(mjx::JitInfo);
  out->size = (int)sizeof(mjx::JitInfo);
  if (!same) return;
  out->hdr = MJX_HDR_HASH;
  out->key = mjx::spec_key<MJX_JIT_ID>();
}
extern "C" __attribute__((visibility("default"))) mjx::StepFn mjx_jit_kernel(int ph) {
  return mjx::phase_kernel<mjx::spec_nr<MJX_JIT_ID>(), MJX_JIT_ID>(ph);
}
