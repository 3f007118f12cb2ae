#!/usr/bin/env bash
# Is the device code of this tree the same as that of another revision?  For every .hip translation unit of csrc/Makefile's SRCS, compile
# the revision and the working tree to device assembly with exactly the flags the Makefile gives that unit (taken from `make -n`, per-target
# additions included) plus --cuda-device-only -S, and compare the two after dropping the __hip_cuid_<hash> lines (they hash the source text)
# and the ordinal of the function in its unit from the block labels (.LBB<function>_<block>, .Lfunc_end<function>: a kernel that is removed
# renumbers every kernel after it).
# Needs hipcc, no GPU.  The gate of a refactor that claims to delete only compile-time-dead code.
#
#   tools/asm_identity.sh <git-rev> [unit.hip ...]       (default: every unit)
#   ASM_IDENTITY_DIR=<dir>  keep the assembly there (the revision's is reused by the next run); default: a temporary folder
#   JOBS=<n>                compilations at a time (default 8)
# Exit status 0: every unit identical.
set -euo pipefail
[ $# -ge 1 ] || { echo "usage: $0 <git-rev> [unit.hip ...]" >&2; exit 2; }
root=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
rev=$(git -C "$root" rev-parse --verify "$1^{commit}"); shift
csrc=toy-cpu-pathtracing_amd/csrc
work=${ASM_IDENTITY_DIR:-$(mktemp -d)}
[ -n "${ASM_IDENTITY_DIR:-}" ] || trap 'rm -rf "$work"' EXIT
mkdir -p "$work"
work=$(cd "$work" && pwd)
jobs=${JOBS:-8}

# the Makefile's own compile lines of <tree>, rewritten to emit device assembly into <out>; a unit whose assembly is there already is left out
asm_commands() {    # <tree> <out> [unit ...]
    local tree=$1 out=$2; shift 2
    make -C "$tree/$csrc" -n -B --no-print-directory | grep -E ' -c -o build/[^ ]+\.hip\.o ' |
        while IFS= read -r line; do
            u=${line##* }
            [ $# -eq 0 ] || [[ " $* " == *" $u "* ]] || continue
            [ -f "$out/$u.s" ] || echo "$line" | sed -E "s# -c -o build/[^ ]+\.o # --cuda-device-only -S -o $out/$u.tmp #; s#\$# \&\& mv $out/$u.tmp $out/$u.s#"
        done
}
compile() {         # <tree> <out> [unit ...]
    local tree=$1 out=$2
    mkdir -p "$out"
    asm_commands "$@" | (cd "$tree/$csrc" && xargs -r -P "$jobs" -d '\n' -I{} sh -c '{}')
}

# the assembly without what differs between two compilations of the same code
clean() { grep -v __hip_cuid_ "$1" | sed -E 's/BB[0-9]+_([0-9]+)/BB_\1/g; s/\.Lfunc_(begin|end)[0-9]+/.Lfunc_\1/g; s/[ \t]+;/ ;/g'; }
# every line of a function's body, prefixed with the function's label
functions() { clean "$1" | awk '/^[^ \t;.][^ \t]*:[ \t]*; @/ { f = $1 } f != "" { print f "\t" $0 } /^\.Lfunc_end/ { f = "" }'; }

base=$work/$rev
rm -rf "$work/tree-$rev" && mkdir -p "$work/tree-$rev"
git -C "$root" archive "$rev" "$csrc" include | tar -x -C "$work/tree-$rev"
compile "$work/tree-$rev" "$base" "$@"
rm -rf "$work/tree-$rev"
cand=$work/worktree
rm -rf "$cand"
compile "$root" "$cand" "$@"

status=0
for s in "$cand"/*.s; do
    [ $# -eq 0 ] || [[ " $* " == *" $(basename "$s" .s) "* ]] || continue
    u=$(basename "$s" .s)
    if [ ! -f "$base/$u.s" ]; then echo "NEW        $u (not in ${rev:0:12})"; status=1
    elif cmp -s <(clean "$base/$u.s") <(clean "$s"); then echo "identical  $u"
    else
        echo "DIFFERENT  $u ($(diff <(clean "$base/$u.s") <(clean "$s") | grep -c '^[<>]') lines), in the functions:"; status=1
        diff <(functions "$base/$u.s") <(functions "$s") | grep '^[<>]' | cut -f1 | cut -c3- | sort -u | c++filt | cut -c1-160 | sed 's/^/             /' || true
    fi
done
[ $# -ne 0 ] || for s in "$base"/*.s; do [ -f "$cand/$(basename "$s")" ] || { echo "MISSING    $(basename "$s" .s)"; status=1; }; done
echo "device assembly vs ${rev:0:12}: $([ $status -eq 0 ] && echo "all units identical" || echo "NOT identical")"
exit $status
