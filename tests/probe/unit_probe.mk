# TEST INFRASTRUCTURE ONLY — libjt_unit_probe.so: sincos_unit and the baked matte sample's local draw in
# both forms (jt_unit_probe.hip, tests/test_gpu_sincos_unit.py). Not linked into libjtrace_hip.so.
#
# The compiler, the flag variables (HIPFLAGS, KFLAGS: the product's, token for token), PKG and HDR are
# Makefile's, included as it is; the command is its first rule's, for the other source.
#
#   make -f unit_probe.mk unit                 ../../julia-raytracer_amd/build/libjt_unit_probe.so
#   make -f unit_probe.mk unit UOUT=/tmp/u.so X="..."   with extra flags somewhere else
include Makefile

UOUT ?= $(PKG)/build/libjt_unit_probe.so

unit: $(UOUT)

# one step, no object file: the library is complete wherever the tree is copied
$(UOUT): jt_unit_probe.hip $(HDR) Makefile unit_probe.mk
	@mkdir -p $(dir $(UOUT))
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) -I$(PKG)/csrc -shared -o $@ jt_unit_probe.hip

.PHONY: unit
