# Builds the C-ABI engine (HIP, gfx950) and the oracle's C restatement.
HIPCC ?= hipcc
ARCH  ?= gfx950
CSRC  := directtrajopt.jl_amd/csrc
# TUNING=1 compiles the A/B switches (environment variables DTO_*) into a SECOND library, libdto_engine_t.so, from objects of
# its own (*.t.o); the product build reads no environment variable
LIB   := directtrajopt.jl_amd/libdto_engine$(if $(TUNING),_t,).so
O     := $(if $(TUNING),t.o,o)
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $(if $(TUNING),-DDTO_TUNING,)
OBJS  := $(addprefix $(CSRC)/,dto_kernels.$(O) dto_small.$(O) dto_sweep_fused.$(O) dto_sweep_gs.$(O) dto_chain64.$(O) dto_tdb.$(O) dto_tdb_mfma.$(O) dto_tdb_kron.$(O) dto_kron.$(O) dto_quadform.$(O) dto_share.$(O) dto_rollout.$(O) dto_dynsolve.$(O) dto_elim.$(O) dto_reduced.$(O) dto_feasible.$(O) dto_newton.$(O) dto_newton_box.$(O) dto_precond.$(O) dto_minimize.$(O) dto_auglag.$(O) dto_hess_product.$(O) dto_hostxfer.$(O) dto_comm.$(O) dto_create.$(O) dto_engine.$(O))

all: $(LIB)

# header dependencies come from the compiler (-MMD -MP writes a .d file beside every object)
$(CSRC)/%.$(O): $(CSRC)/%.hip
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@

$(CSRC)/%.$(O): $(CSRC)/%.cpp
	$(HIPCC) $(HIPFLAGS) -MMD -MP -x hip -c $< -o $@

-include $(OBJS:.o=.d)

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lpthread -ldl

clean:
	rm -f $(CSRC)/*.o $(CSRC)/*.d directtrajopt.jl_amd/libdto_engine.so directtrajopt.jl_amd/libdto_engine_t.so

.PHONY: all clean
