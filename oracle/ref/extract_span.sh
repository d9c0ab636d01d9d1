#!/bin/sh
# extract_span.sh SRC FIRST LAST FIRST_RE LAST_RE OUT [MUST_CONTAIN_RE]
# Copies lines FIRST..LAST of the reference file SRC to OUT (under oracle/_ref/, git-ignored).
# Fails, writing nothing, unless line FIRST matches FIRST_RE, line LAST matches LAST_RE, the braces
# of the span balance (so the last line closes what the first opened) and, when given, some line of
# the span matches MUST_CONTAIN_RE.  The patterns are identifiers to anchor on, nothing more.
set -eu
src=$1; first=$2; last=$3; fre=$4; lre=$5; out=$6; must=${7:-}
awk -v a="$first" -v b="$last" -v fre="$fre" -v lre="$lre" -v must="$must" -v src="$src" '
    function fail(msg) { printf "span guard: %s:%d-%d: %s\n", src, a, b, msg > "/dev/stderr"; bad = 1 }
    NR == a && $0 !~ fre { fail("first line does not match /" fre "/: " $0) }
    NR == b && $0 !~ lre { fail("last line does not match /" lre "/: " $0) }
    NR >= a && NR <= b {
        line = $0
        sub(/\/\/.*$/, "", line)
        open += gsub(/\{/, "{", line); close_ += gsub(/\}/, "}", line)
        if (must != "" && $0 ~ must) seen = 1
        print
    }
    END {
        if (NR < b) fail("file has only " NR " lines")
        if (open != close_) fail("braces do not balance (" open " opened, " close_ " closed)")
        if (must != "" && !seen) fail("no line matches /" must "/")
        exit bad
    }' "$src" > "$out.tmp" || { rm -f "$out.tmp"; exit 1; }
mv "$out.tmp" "$out"
