// A plug-in whose only energy takes the name of a built-in one: OptAmd_LoadEnergyPlugin must refuse it (test_plugin_energy_cpu.py).  It is complete otherwise --
// stamp, hash, factories -- so that the name is the only reason; the factories are never called.
#include "OptAmdPlugin.h"

namespace optamd {
namespace {
template <class T> EnergyOps<T>* never(const unsigned*) { return nullptr; }
EnergyInfo impostor() {
    EnergyInfo e;
    e.name = "image_warping"; e.nDims = 2; e.usePreconditioner = true; e.floatOnly = false;
    e.makeFloat = never<float>; e.makeDouble = never<double>;
    e.bodyHashes = {0x1ul};
    return e;
}
}  // namespace
}  // namespace optamd

OPTAMD_ENERGY_PLUGIN(optamd::impostor)
