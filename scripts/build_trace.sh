# Instrumented (-DTAVSR_GEMM_TRACE) build of the library for profiles/gemm_trace.py; the product build is untouched.
set -e
cd "$(dirname "$0")/../tailored-avsr_amd/csrc"
make -j8 > /dev/null
mkdir -p build_trace ../tavsr/lib_trace
for f in gemm gemm_conv; do      # the two units that hold gemm_glds.h's ring
  hipcc -DTAVSR_GEMM_TRACE -O3 --offload-arch=gfx950 -fPIC -std=c++17 -I../../include -I. -Wall -Wno-unused-function -c $f.hip -o build_trace/$f.o
done
objs=$(ls build/*.o | grep -v -e build/gemm.o -e build/gemm_conv.o)
hipcc --offload-arch=gfx950 -shared -fPIC -o ../tavsr/lib_trace/libtavsr_hip.so build_trace/gemm.o build_trace/gemm_conv.o $objs
echo built ../tavsr/lib_trace/libtavsr_hip.so
