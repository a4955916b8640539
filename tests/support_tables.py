"""The strategies and the builders by name, once for the whole suite.

A test module that runs a subset takes a subset (`{k: KERNELS[k] for k in (...)}`), one that adds an entry adds it
(`dict(WALKS, auto=rtow.KERNEL_AUTO)`); the key order below is the order of the test ids parametrised over these maps.
"""
import rtow

KERNELS = {"brute": rtow.KERNEL_BRUTE, "bvh": rtow.KERNEL_BVH, "grid": rtow.KERNEL_GRID, "bvh4": rtow.KERNEL_BVH4,
           "reftree": rtow.KERNEL_REFTREE}
# the four walks of the fast build and of the queries (REFTREE is the strict render's and the strict closest hit's only)
WALKS = {k: KERNELS[k] for k in ("brute", "bvh", "grid", "bvh4")}
BUILDERS = {"host": rtow.BUILDER_HOST_SAH, "device": rtow.BUILDER_DEVICE_LBVH}
