# build_variant.sh NAME "-DFLAGS..." [REV]
#   -> triangles-sdf-cpu-raytracing_amd/lib/var_NAME.so (A/B experiments).
# The flags apply to one unit, csrc/$VAR_UNIT.hip (default rt_device, the render
# kernels; VAR_UNIT=rt_bvhgpu: the BVH builder); the other objects are the
# shipping build's (the Makefile's object list).
# With REV (a git revision), the unit and its headers are taken from that
# revision instead of the working tree (A/B against a committed state). The
# rest links from this tree's objects, so the revision must split csrc/ into
# the same units: where it does not, the script stops and says so, and the
# revision's library is built from a checkout of its own (git worktree, make).
set -e
R=$(cd $(dirname $0)/.. && pwd)
P=$R/triangles-sdf-cpu-raytracing_amd
cd $P
mkdir -p build/var lib
U=${VAR_UNIT:-rt_device}
SRC=csrc/$U.hip
if [ -n "$3" ]; then
  THEN=$(git -C $R ls-tree --name-only $3 triangles-sdf-cpu-raytracing_amd/csrc/ | grep -E '\.(hip|cpp)$' | xargs -n1 basename | sort | tr '\n' ' ')
  NOW=$(ls csrc/*.hip csrc/*.cpp | xargs -n1 basename | sort | tr '\n' ' ')
  if [ "$THEN" != "$NOW" ]; then
    echo "build_variant.sh: revision $3 splits csrc/ into other units than this tree:" >&2
    echo "  $3: $THEN" >&2
    echo "  tree: $NOW" >&2
    echo "its unit cannot link against this tree's objects; build its library from a checkout of its own (git worktree add, make) and select it through RTAMD_LIB" >&2
    exit 1
  fi
  S=build/var/src_$1
  rm -rf $S && mkdir -p $S/include $S/p/csrc
  for f in $(git -C $R ls-tree --name-only $3 triangles-sdf-cpu-raytracing_amd/csrc/); do
    case $f in *.h|*.hip) git -C $R show $3:$f > $S/p/csrc/$(basename $f) ;; esac
  done
  git -C $R show $3:include/rtamd.h > $S/include/rtamd.h
  SRC=$S/p/csrc/$U.hip
fi
# the shipping build's flags (the Makefile's HIPFLAGS), plus RT_AB_ENV: a
# variant reads the RTAMD_* A/B switches from the environment (the shipping
# library does not, csrc/rt_host.h ab_env)
HIPF="$(make -s print-hipflags) -DRT_AB_ENV=1"
/opt/rocm/bin/hipcc $HIPF $2 -c -o build/var/${U}_$1.o $SRC
# the variant's own build id: the tree's id + its name and a hash of its
# flags and revision, so a bench line from a variant never passes for the
# shipping library's
make -s build/rt_buildid.o
BASE=$(sed -n 's/.*return "\([0-9a-f]*\)".*/\1/p' build/rt_buildid.cpp)
VH=$(printf '%s|%s|%s|%s' "$2" "$3" "$VAR_UNIT" "$HIPF" | sha256sum | cut -c1-8)
printf 'extern "C" const char *rt_build_id(void) { return "%s+%s:%s"; }\n' "$BASE" "$1" "$VH" > build/var/rt_buildid_$1.cpp
g++ -fPIC -c -o build/var/rt_buildid_$1.o build/var/rt_buildid_$1.cpp
OBJS=$(make -s print-objs | tr ' ' '\n' | grep -v -e "^build/$U.o\$" -e '^build/rt_buildid.o$')
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -fPIC -o lib/var_$1.so $OBJS build/var/${U}_$1.o build/var/rt_buildid_$1.o -lgomp -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
