"""Known-answer cases for Go's encoding/csv Reader with LazyQuotes = true (Reader.LazyQuotes(), csvplus.go:982-987), in the
format of go_csv_reader_cases.py: (name, input bytes, options, expected records, (error_kind, error_record) or None).

These are NOT recorded Go output: Go is not run here and encoding/csv is not part of the reference tree.  They restate the
stdlib's rules and the lazy cases of its reader tests (LazyQuotes, BareQuotes, BareDoubleQuotes, LazyQuoteWithTrailingCRLF)
plus the line-end and comment situations the device's separator scan has to get right; every expectation is the output of
tests/lazy_csv_model.py, whose strict mode is tied to the pinned oracle.
Two cases whose records differ in length carry fpr -1 (any field count): with csv.Reader's zero value the second record
would be ErrFieldCount, which the last case pins on its own.
"""
FIELDS = 3

LAZY_CASES = [
    ("LazyQuotes", b'a "word","1"2",a","b', {}, [[b'a "word"', b'1"2', b'a"', b"b"]], None),
    ("BareQuotes", b'a "word","1"2",a"', {}, [[b'a "word"', b'1"2', b'a"']], None),
    ("BareDoubleQuotes", b'a""b,c', {}, [[b'a""b', b"c"]], None),
    ("LazyQuoteWithTrailingCRLF", b'"foo"bar"\r\n', {}, [[b'foo"bar']], None),
    ("OddQuotes", b'"""""""', {}, [[b'"""']], None),
    ("EOFInQuotes", b'a,"b\nc', {}, [[b"a", b"b\nc"]], None),
    ("QuotedTrailingCRCR", b'"field"\r\r', {}, [[b'field"\r']], None),
    ("OpenQuoteCRLF", b'"a\r\n', {}, [[b"a\n"]], None),
    ("OpenQuoteCR", b'"abc\r', {}, [[b"abc"]], None),
    ("QuoteCRLFThenRecord", b'a,"b"\r\nc', {"fpr": -1}, [[b"a", b"b"], [b"c"]], None),
    ("QuoteInUnquoted", b'a"b,c\nd,e\n', {}, [[b'a"b', b"c"], [b"d", b"e"]], None),
    ("NeverClosed", b'"a"b\nc,d\n', {}, [[b'a"b\nc,d\n']], None),
    ("QuoteCRCRLF", b'"a"\r\r\nb"\nc\n', {}, [[b'a"\r\nb'], [b"c"]], None),
    ("QuoteCRQuote", b'"a"\r"b",c\n', {}, [[b'a"\r"b', b"c"]], None),
    ("EscapedThenLone", b'a,"b""c"d",e\n', {}, [[b"a", b'b"c"d', b"e"]], None),
    ("EmptyLastThenOpen", b'"a",\n"b\n', {"fpr": -1}, [[b"a", b""], [b"b\n"]], None),
    ("BlankLinesInQuotes", b'a,b\n\n"c\n\nd",e\n', {}, [[b"a", b"b"], [b"c\n\nd", b"e"]], None),
    ("TrimBeforeQuote", b'x,  "a"b",c\n', {"trim": True}, [[b"x", b'a"b', b"c"]], None),
    ("NoTrimBeforeQuote", b'x,  "a"b",c\n', {}, [[b"x", b'  "a"b"', b"c"]], None),
    ("TrimTabCRBeforeQuote", b'x,\t\r"q"z",y\n', {"trim": True}, [[b"x", b'q"z', b"y"]], None),
    ("CommentWithQuote", b'a,b\n# "odd\nc,d\n', {"comment": b"#"}, [[b"a", b"b"], [b"c", b"d"]], None),
    ("CommentCharInQuotes", b'"a\n#b",c\n', {"comment": b"#"}, [[b"a\n#b", b"c"]], None),
    ("TrimThenCommentChar", b" #x\n#y\n", {"trim": True, "comment": b"#"}, [[b"#x"]], None),
    ("FieldCountAfterLazy", b'a,b\n"c"d\n', {"fpr": 0}, [[b"a", b"b"]], (FIELDS, 1)),
]
