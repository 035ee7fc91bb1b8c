// strpred.go — the conditions and values that look inside a string, for the cgo shim: StrCmp / HasPrefix / HasSuffix /
// Contains as declarative predicates (cph_filter_rows ops CPH_PRED_STR_LT.., CPH_PRED_HAS_PREFIX / HAS_SUFFIX / CONTAINS) and
// Substr as a Map template part (CPH_MAP_SLICE).
//
// NOT COMPILED IN THIS REPOSITORY, like gpu.go and join.go: the build image has no Go toolchain.  The same constructors are
// compiled and tested in C++ (csvplus_amd/host/csvplus.hpp, tests/cpp/test_strpred_facade.cpp); this file is the source a
// maintainer vets (gofmt / go vet) and adapts.  Drop it into the csvplus package directory beside gpu.go.
package csvplus

/*
#include <stdint.h>
#include "csvplus_hip.h"
*/
import "C"

import (
	"math"
	"strings"
	"unsafe"
)

// Rel is a relation of StrCmp, in the order of CPH_PRED_STR_LT .. CPH_PRED_STR_GT.
type Rel int

const (
	LT Rel = iota
	LE
	EQ
	NE
	GE
	GT
)

// strTerm is the declarative form of one string condition: what Filter finds in the side table of named predicates
// (INTEGRATION.md) instead of an opaque closure.
type strTerm struct {
	op      C.int32_t // CPH_PRED_STR_LT + rel, CPH_PRED_HAS_PREFIX, CPH_PRED_HAS_SUFFIX or CPH_PRED_CONTAINS
	column  string
	literal string
}

// strTerms remembers the term behind every func the constructors below hand out, keyed by the func's pointer; guarded by gpuMu.
var strTerms = map[uintptr]strTerm{}

func remember(f func(Row) bool, t strTerm) func(Row) bool {
	gpuMu.Lock()
	strTerms[*(*uintptr)(unsafe.Pointer(&f))] = t
	gpuMu.Unlock()
	return f
}

// StrCmp is `row[column] REL literal`: Go's string comparison, bytewise.  A row without the column is false under every
// relation, NE included.
func StrCmp(column string, rel Rel, literal string) func(Row) bool {
	f := func(row Row) bool {
		v, found := row[column]
		if !found {
			return false
		}
		c := strings.Compare(v, literal)
		switch rel {
		case LT:
			return c < 0
		case LE:
			return c <= 0
		case EQ:
			return c == 0
		case NE:
			return c != 0
		case GE:
			return c >= 0
		}
		return c > 0
	}
	return remember(f, strTerm{C.CPH_PRED_STR_LT + C.int32_t(rel), column, literal})
}

// HasPrefix is strings.HasPrefix(row[column], literal); a row without the column is false.
func HasPrefix(column, literal string) func(Row) bool {
	f := func(row Row) bool { v, found := row[column]; return found && strings.HasPrefix(v, literal) }
	return remember(f, strTerm{C.CPH_PRED_HAS_PREFIX, column, literal})
}

// HasSuffix is strings.HasSuffix(row[column], literal); a row without the column is false.
func HasSuffix(column, literal string) func(Row) bool {
	f := func(row Row) bool { v, found := row[column]; return found && strings.HasSuffix(v, literal) }
	return remember(f, strTerm{C.CPH_PRED_HAS_SUFFIX, column, literal})
}

// Contains is strings.Contains(row[column], literal); a row without the column is false.
func Contains(column, literal string) func(Row) bool {
	f := func(row Row) bool { v, found := row[column]; return found && strings.Contains(v, literal) }
	return remember(f, strTerm{C.CPH_PRED_CONTAINS, column, literal})
}

// appendStrTerm appends the term's three ops to a postfix program: the term on staged column `col`, a LIKE "1" on staged column
// `flag`, and ALL 2.  `flag` is the column's PRESENCE FLAG: the stager writes "1" for a row that has the column and "" for
// one that lacks it.  No stand-in value is false under all nine ops (NE wants it equal to the literal, LT above it), so
// presence travels as a column of its own.  lit and one must be C memory (or pinned for the call): cgo pointer rules.
func appendStrTerm(ops []C.cph_pred_op, t strTerm, col, flag int, lit unsafe.Pointer, one unsafe.Pointer) []C.cph_pred_op {
	var term, like, all C.cph_pred_op
	term.op, term.arg = t.op, C.int32_t(col)
	term.value.data, term.value.len = (*C.uint8_t)(lit), C.uint64_t(len(t.literal))
	like.op, like.arg = C.CPH_PRED_LIKE, C.int32_t(flag)
	like.value.data, like.value.len = (*C.uint8_t)(one), 1
	all.op, all.arg = C.CPH_PRED_ALL, 2
	return append(ops, term, like, all)
}

// SubstrPart is the template part `row[column][from:to]` with Python's slice rules: a negative index counts from the end,
// both ends are clamped into the value (where Go itself would panic), from >= to gives "", To == math.MaxInt64 means "to
// the end".  Bytes, not runes, as Go's own slice expression.
type SubstrPart struct {
	Column   string
	From, To int64
}

// Substr(column, from) is row[column][from:]; Substr(column, from, to) is row[column][from:to].
func Substr(column string, from int64, to ...int64) SubstrPart {
	p := SubstrPart{column, from, math.MaxInt64}
	if len(to) > 0 {
		p.To = to[0]
	}
	return p
}

// Of is the part on one value, on the host: what the device computes for a batch.
func (p SubstrPart) Of(v string) string {
	clamp := func(i int64) int64 {
		n := int64(len(v))
		if i < 0 {
			i += n
			if i < 0 {
				return 0
			}
			return i
		}
		if i > n {
			return n
		}
		return i
	}
	f, t := clamp(p.From), clamp(p.To)
	if t <= f {
		return ""
	}
	return v[f:t]
}

// piece fills a cph_map_piece for staged column `col`; sl must be C memory that lives until cph_map_format returns.
func (p SubstrPart) piece(col int, sl *C.cph_map_slice) C.cph_map_piece {
	sl.from, sl.to = C.int64_t(p.From), C.int64_t(p.To)
	var piece C.cph_map_piece
	piece.kind, piece.arg = C.CPH_MAP_SLICE, C.int32_t(col)
	piece.value.data, piece.value.len = (*C.uint8_t)(unsafe.Pointer(sl)), 16
	return piece
}
