# Top-level build: the gfx950 product library, the oracle, the reference build.
#   make            libmtcp_gpu.so + oracle/libmtcp_oracle.so
#   make ref        oracle/_ref (needs /root/reference; this container only)
#   make golden     regenerate tests/golden from the reference
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
HIPFLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-result
LIB      := mtcp_amd/lib/libmtcp_gpu.so
SRCS     := mtcp_amd/csrc/mtcp_gpu.hip mtcp_amd/csrc/pktgen.hip mtcp_amd/csrc/rxq.hip
DEPS     := $(SRCS) mtcp_amd/csrc/dispatch.hpp mtcp_amd/csrc/rx_kernels.hpp mtcp_amd/csrc/rx_wave.hpp mtcp_amd/csrc/rx_span.hpp mtcp_amd/csrc/host_call.hpp mtcp_amd/csrc/stage_layout.hpp mtcp_amd/csrc/host_copy.hpp mtcp_amd/csrc/park.hpp mtcp_amd/csrc/wait.hpp mtcp_amd/csrc/ctx_internal.hpp mtcp_amd/csrc/flow_kernels.hpp mtcp_amd/csrc/flowtab_kernels.hpp mtcp_amd/csrc/group_kernels.hpp mtcp_amd/csrc/rcvwalk_kernels.hpp mtcp_amd/csrc/rcvcopy_kernels.hpp mtcp_amd/csrc/rcvread_kernels.hpp mtcp_amd/csrc/rcvread_step.hpp mtcp_amd/csrc/sndwrite_kernels.hpp mtcp_amd/csrc/sndwrite_step.hpp mtcp_amd/csrc/ackwalk_kernels.hpp mtcp_amd/csrc/ackgen_kernels.hpp mtcp_amd/csrc/ackgen_step.hpp mtcp_amd/csrc/datagen_kernels.hpp mtcp_amd/csrc/datagen_step.hpp mtcp_amd/csrc/rtosweep_kernels.hpp mtcp_amd/csrc/rto_step.hpp mtcp_amd/csrc/ack_step.hpp mtcp_amd/csrc/tcpopt_kernels.hpp mtcp_amd/csrc/steer_kernels.hpp mtcp_amd/csrc/txbuild_kernels.hpp mtcp_amd/csrc/txseg_kernels.hpp include/mtcp_gpu.h include/mtcp_gpu_pktgen.h include/mtcp_gpu_rxq.h include/mtcp_gpu_tcpopt.h include/mtcp_gpu_steer.h include/mtcp_gpu_txbuild.h include/mtcp_gpu_txseg.h include/mtcp_gpu_flowtab.h include/mtcp_gpu_group.h include/mtcp_gpu_rcvwalk.h include/mtcp_gpu_rcvcopy.h include/mtcp_gpu_ackwalk.h include/mtcp_gpu_ackgen.h include/mtcp_gpu_datagen.h include/mtcp_gpu_rcvread.h include/mtcp_gpu_rtosweep.h include/mtcp_gpu_sndwrite.h

.PHONY: all lib oracle ref golden examples clean tools

all: lib oracle

lib: $(LIB)

$(LIB): $(DEPS)
	mkdir -p mtcp_amd/lib
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(SRCS)

oracle:
	$(MAKE) -C oracle

ref:
	$(MAKE) -C oracle ref

golden:
	$(MAKE) -C oracle golden

clean:
	rm -f $(LIB) tests/c/libmtcp_gpu_testing.so tests/c/rxloop tests/c/admit_test tests/c/park_test tests/c/asan_host tools/libstream_ceiling.so tools/libtcpopt_pattern.so tools/libsteer_pattern.so tools/libtxbuild_pattern.so tools/libtxseg_pattern.so tools/libflowtab_pattern.so tools/libgroup_pattern.so tools/librcvwalk_pattern.so tools/librcvcopy_pattern.so tools/libackwalk_pattern.so tools/libackgen_pattern.so tools/libdatagen_pattern.so tools/librtosweep_pattern.so tools/librcvread_pattern.so tools/libsndwrite_pattern.so
	$(MAKE) -C oracle clean

# the probe tools instantiate rx_kernel's profiling / timing-probe variants
# (ABL, STAMP, XSKIP), which only a -DMTCP_GPU_TESTING build allows
TOOLFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -w -DMTCP_GPU_TESTING

tools/rx_variants: tools/rx_variants.hip mtcp_amd/csrc/rx_kernels.hpp $(LIB)
	$(HIPCC) $(TOOLFLAGS) -o $@ $< -Lmtcp_amd/lib -lmtcp_gpu -Wl,-rpath,'$$ORIGIN/../mtcp_amd/lib'

tools/hbm_ceiling: tools/hbm_ceiling.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -w -o $@ $<

tools/store_probe: tools/store_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -w -o $@ $<

tools/pcie_probe: tools/pcie_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -w -o $@ $<

tools: tools/rx_variants tools/hbm_ceiling tools/store_probe tools/pcie_probe tools/wave_probe

# The test-only library: mtcp_gpu_debug_stall (tests/c/mtcp_gpu_testing.h),
# fault injection kept out of the product library
TESTLIB := tests/c/libmtcp_gpu_testing.so
$(TESTLIB): tests/c/gpu_testing.hip tests/c/mtcp_gpu_testing.h include/mtcp_gpu.h $(LIB)
	$(HIPCC) $(HIPFLAGS) -Iinclude -shared -o $@ $< -Lmtcp_amd/lib -lmtcp_gpu -Wl,-rpath,'$$ORIGIN/../../mtcp_amd/lib'

# gpu_module.c driven by the RunMainLoop rx harness; the
# mTCP types come from the test doubles in tests/c/mtcp_double.  A test
# build (-DMTCP_GPU_TESTING): the fault-injection variables are read.
tests/c/rxloop: tests/c/rxloop.c mtcp_amd/io_module/gpu_module.c mtcp_amd/io_module/gpu_topo.h include/mtcp_gpu_rxq.h oracle/mtcp_oracle.c $(LIB) $(TESTLIB)
	gcc -std=gnu99 -O3 -Wall -pthread -DMTCP_GPU_TESTING -Itests/c/mtcp_double -Itests/c -Iinclude -o $@ tests/c/rxloop.c \
	    mtcp_amd/io_module/gpu_module.c oracle/mtcp_oracle.c -Lmtcp_amd/lib -Ltests/c -lmtcp_gpu -lmtcp_gpu_testing -ldl \
	    -Wl,-rpath,'$$ORIGIN/../../mtcp_amd/lib' -Wl,-rpath,'$$ORIGIN'

# park.hpp's best fit and caps, run on the GPU box (tests/test_gpu_bounded.py)
tests/c/park_test: tests/c/park_test.hip mtcp_amd/csrc/park.hpp
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -Wall -o $@ $<

# the C ABI's host code under AddressSanitizer (host side only: the pool has
# no GPU ASan), run on the GPU box by tests/test_gpu_bounded.py
ASAN_SRCS := tests/c/asan_host.hip mtcp_amd/csrc/mtcp_gpu.hip mtcp_amd/csrc/rxq.hip mtcp_amd/csrc/pktgen.hip
tests/c/asan_host: $(ASAN_SRCS) $(DEPS)
	$(HIPCC) --offload-arch=$(ARCH) -O2 -g -std=c++17 -Wall -Wno-unused-result -Xarch_host -fsanitize=address \
	    -Xarch_host -fno-omit-frame-pointer -o $@ $(ASAN_SRCS)

# the admission / limit logic of gpu_module.c, unit-tested on the CPU
tests/c/admit_test: tests/c/admit_test.c mtcp_amd/io_module/gpu_module.c $(LIB)
	gcc -std=gnu99 -O1 -Wall -pthread -Itests/c/mtcp_double -Iinclude -o $@ tests/c/admit_test.c \
	    oracle/mtcp_oracle.c -Lmtcp_amd/lib -lmtcp_gpu -Wl,-rpath,'$$ORIGIN/../../mtcp_amd/lib'

tools/wave_probe: tools/wave_probe.hip mtcp_amd/csrc/rx_span.hpp mtcp_amd/csrc/rx_wave.hpp mtcp_amd/csrc/rx_kernels.hpp $(LIB)
	$(HIPCC) $(TOOLFLAGS) -o $@ $< -Lmtcp_amd/lib -lmtcp_gpu -Wl,-rpath,'$$ORIGIN/../mtcp_amd/lib'

tools/occ_probe: tools/occ_probe.hip mtcp_amd/csrc/rx_kernels.hpp $(LIB)
	$(HIPCC) $(TOOLFLAGS) -o $@ $< -Lmtcp_amd/lib -lmtcp_gpu -Wl,-rpath,'$$ORIGIN/../mtcp_amd/lib'

tools/tx_probe: tools/tx_probe.hip mtcp_amd/csrc/rx_kernels.hpp $(LIB)
	$(HIPCC) $(TOOLFLAGS) -o $@ $< -Lmtcp_amd/lib -lmtcp_gpu -Wl,-rpath,'$$ORIGIN/../mtcp_amd/lib'

# bench.py's read-ceiling leg (measurement only, not the product)
tools/libstream_ceiling.so: tools/stream_ceiling.hip
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/tcpopt_bench.py's yardstick: the option kernel's loads and stores
# without its walks (measurement only, not the product)
tools/libtcpopt_pattern.so: tools/tcpopt_pattern.hip
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/steer_bench.py's yardstick: the steer passes' loads and stores on the
# same grids without any ranking (measurement only, not the product)
tools/libsteer_pattern.so: tools/steer_pattern.hip
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/txbuild_bench.py's yardstick: the frame builder's loads and stores on
# the same grid without sums and shifts (measurement only, not the product)
tools/libtxbuild_pattern.so: tools/txbuild_pattern.hip mtcp_amd/csrc/txbuild_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp mtcp_amd/csrc/dispatch.hpp include/mtcp_gpu_txbuild.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/txseg_bench.py's yardstick: the segment passes' loads and stores on the
# same grids without the arithmetic and the search (measurement only, not the
# product)
tools/libtxseg_pattern.so: tools/txseg_pattern.hip mtcp_amd/csrc/txseg_kernels.hpp mtcp_amd/csrc/txbuild_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_txseg.h include/mtcp_gpu_txbuild.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/flowtab_bench.py's yardstick: the lookup's record loads, one 16 B gather
# at a precomputed slot per TCP_OK record and its stores on the same grid,
# without hashing, comparing and probing; and one host core walking a chained
# table over the same records (measurement only, not the product)
tools/libflowtab_pattern.so: tools/flowtab_pattern.hip mtcp_amd/csrc/flowtab_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_flowtab.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/group_bench.py's yardstick: the group passes' loads and stores on the
# same grids without any ranking (measurement only, not the product)
tools/libgroup_pattern.so: tools/group_pattern.hip mtcp_amd/csrc/group_kernels.hpp mtcp_amd/csrc/steer_kernels.hpp mtcp_amd/csrc/flow_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_flowtab.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/rcvwalk_bench.py's yardsticks: the walk's loads and stores on the same
# grids without the walk, the same walk as a plain loop on one host core, and
# the walk kernel at other thresholds (measurement only, not the product)
tools/librcvwalk_pattern.so: tools/rcvwalk_pattern.hip mtcp_amd/csrc/rcvwalk_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_rcvwalk.h include/mtcp_gpu_group.h include/mtcp_gpu_tcpopt.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/rcvcopy_bench.py's yardsticks: the copy's loads and stores on the same
# grids without plan, shift or ordering, the plan's step functions as a plain
# loop on the host, and one host core doing the same copies with memcpy
# (measurement only, not the product)
tools/librcvcopy_pattern.so: tools/rcvcopy_pattern.hip mtcp_amd/csrc/rcvcopy_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp mtcp_amd/csrc/dispatch.hpp include/mtcp_gpu_rcvcopy.h include/mtcp_gpu_rcvwalk.h include/mtcp_gpu_group.h include/mtcp_gpu_tcpopt.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/ackwalk_bench.py's yardsticks: the ACK walk's loads and stores on the
# same grids without the walk, and the same walk (ack_step.hpp compiled for the
# host) as a plain loop on one host core (measurement only, not the product)
tools/libackwalk_pattern.so: tools/ackwalk_pattern.hip mtcp_amd/csrc/ackwalk_kernels.hpp mtcp_amd/csrc/ack_step.hpp mtcp_amd/csrc/rcvwalk_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_ackwalk.h include/mtcp_gpu_rcvwalk.h include/mtcp_gpu_group.h include/mtcp_gpu_tcpopt.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/ackgen_bench.py's yardsticks: the ACK generation's loads and stores on
# the same grids without the fold, the plan and the record arithmetic, and the
# library's launches with the plan kernel's lane threshold as a parameter
# (measurement only, not the product)
tools/libackgen_pattern.so: tools/ackgen_pattern.hip mtcp_amd/csrc/ackgen_kernels.hpp mtcp_amd/csrc/ackgen_step.hpp mtcp_amd/csrc/txseg_kernels.hpp mtcp_amd/csrc/txbuild_kernels.hpp mtcp_amd/csrc/rcvwalk_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_ackgen.h include/mtcp_gpu_ackwalk.h include/mtcp_gpu_rcvwalk.h include/mtcp_gpu_txseg.h include/mtcp_gpu_txbuild.h include/mtcp_gpu_group.h include/mtcp_gpu_tcpopt.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/datagen_bench.py's yardstick: the data generation's two kernels' loads
# and stores on the same grids without the fold, the status chain and the
# commit arithmetic (measurement only, not the product)
tools/libdatagen_pattern.so: tools/datagen_pattern.hip mtcp_amd/csrc/datagen_kernels.hpp mtcp_amd/csrc/datagen_step.hpp mtcp_amd/csrc/ackgen_step.hpp mtcp_amd/csrc/txbuild_kernels.hpp mtcp_amd/csrc/rcvwalk_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_datagen.h include/mtcp_gpu_ackgen.h include/mtcp_gpu_ackwalk.h include/mtcp_gpu_rcvwalk.h include/mtcp_gpu_txseg.h include/mtcp_gpu_txbuild.h include/mtcp_gpu_group.h include/mtcp_gpu_tcpopt.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/rcvread_bench.py's yardstick: the read's copy units on the copy kernel's
# grid, no plan, no search, no shift (not the product)
tools/librcvread_pattern.so: tools/rcvread_pattern.hip mtcp_amd/csrc/rcvread_kernels.hpp mtcp_amd/csrc/rcvread_step.hpp mtcp_amd/csrc/rcvcopy_kernels.hpp mtcp_amd/csrc/steer_kernels.hpp mtcp_amd/csrc/flow_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_rcvread.h include/mtcp_gpu_rcvcopy.h include/mtcp_gpu_rcvwalk.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/sndwrite_bench.py's yardstick: the write's copy units on the copy kernel's
# grid, no plan, no search, no shift, no move (not the product)
tools/libsndwrite_pattern.so: tools/sndwrite_pattern.hip mtcp_amd/csrc/sndwrite_kernels.hpp mtcp_amd/csrc/sndwrite_step.hpp mtcp_amd/csrc/rcvread_kernels.hpp mtcp_amd/csrc/rcvread_step.hpp mtcp_amd/csrc/rcvcopy_kernels.hpp mtcp_amd/csrc/steer_kernels.hpp mtcp_amd/csrc/flow_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_sndwrite.h include/mtcp_gpu_datagen.h include/mtcp_gpu_ackwalk.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# tools/rtosweep_bench.py's yardsticks: the sweep's loads and stores on the same
# grids without the step arithmetic and the ranking, and the sweep's launches
# with the due test's form as a parameter (measurement only, not the product)
tools/librtosweep_pattern.so: tools/rtosweep_pattern.hip mtcp_amd/csrc/rtosweep_kernels.hpp mtcp_amd/csrc/rto_step.hpp mtcp_amd/csrc/steer_kernels.hpp mtcp_amd/csrc/flow_kernels.hpp mtcp_amd/csrc/txbuild_kernels.hpp mtcp_amd/csrc/rx_kernels.hpp include/mtcp_gpu_rtosweep.h include/mtcp_gpu_datagen.h include/mtcp_gpu_ackwalk.h include/mtcp_gpu_txseg.h include/mtcp_gpu.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

tools/sector_probe: tools/sector_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -w -o $@ $<
