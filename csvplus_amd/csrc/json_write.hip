// json_write.hip — ToJSON (csvplus.go:446-480): rows as a JSON array of objects, written on the device.
//
//   cph_json_write_rows  '[', then every row as json.Encoder.Encode writes it with SetIndent("", "") and
//                        SetEscapeHTML(false) — one compact object and '\n' — with ',' in front of every row but the
//                        first, then ']' (no rows: "[]").  A Row is a map[string]string: Go writes its keys sorted by
//                        byte order, so the columns are sorted by name on the host and the kernels see them in that order.
//
// Strings (keys and values alike) are escaped as Go >= 1.22 encoding/json appendString does with escapeHTML false,
// restated from the Go standard library:
//   * 0x20..0x7F other than '"' and '\\' are copied (DEL, '<', '>' and '&' included); '"' -> \" and '\\' -> \\;
//   * 0x08 0x0C 0x0A 0x0D 0x09 -> \b \f \n \r \t (the Go >= 1.22 form: earlier releases wrote \u0008 and \u000c);
//     every other byte below 0x20 -> \u00XX with lowercase hex;
//   * bytes >= 0x80 are decoded as utf8.DecodeRuneInString does: a valid sequence is copied (a literal U+FFFD too),
//     U+2028 / U+2029 become \u2028 / \u2029, an invalid or truncated sequence becomes \ufffd and the decoder moves on
//     by ONE byte (overlong forms, surrogates ED A0..BF, leads C0 C1 F5..FF, stray continuation bytes).
//
// The pipeline of the two-pass CSV writer (materialize.hip): k_json_lens (bytes per record + which fields need escaping,
// 8 bytes at a time) -> exclusive scan -> k_json_copy (a tile's records assembled in LDS, streamed out with 16-byte
// stores; a tile beyond the stage writes its records to global memory itself).  A field without any byte to escape is
// copied 8 bytes at a time; only flagged fields take the per-byte escape and UTF-8 path.  The key fragments
// ({"k1":"  ,"k2":"  ...) are rendered once on the host and read by every record from a small device block.
#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <string>

#include "materialize_device.hpp"

namespace cph {

// A JSON record is ~2.5x its CSV record (a 6-column README-chain row: ~110 bytes against ~45): a 256-record tile needs
// ~28 KB, beyond the CSV writer's 16 KB stage.  32 KB keeps the common tile in LDS at 4-5 workgroups per CU.
constexpr int kJsonStage = 32 * 1024;

// Fragment c = (c ? ',' : '{') + '"' + escaped name of (sorted) column c + "\":\"" is bytes [off[c], off[c + 1]).
struct JsonKeys {
    const uint8_t* bytes;
    uint32_t off[kMaxKeyCols + 1];
    uint32_t fixed;   // bytes of a record besides its values and its leading ',': the fragments, a closing '"' per value, "}\n"
};

// 0x80 in every byte of w that is not copied as it is: < 0x20, '"', '\\', >= 0x80 (exact per byte: no carry crosses a byte)
__device__ __forceinline__ uint64_t json_special8(uint64_t w) {
    const uint64_t k = 0x7F7F7F7F7F7F7F7Full, h = 0x8080808080808080ull;
    const uint64_t ctrl = ~(((w & k) + 0x6060606060606060ull) | w) & h;   // top bit clear and the low 7 bits below 0x20
    return ctrl | (w & h) | eq_mask8(w, 0x2222222222222222ull) | eq_mask8(w, 0x5C5C5C5C5C5C5C5Cull);
}

// the value has no byte to escape (chunk0 = its first 8 bytes, already loaded)
__device__ __forceinline__ bool json_clean(const DevCol& col, uint64_t begin, uint64_t len, uint64_t chunk0) {
    uint64_t hit = 0;
    const int nchunks = (int)((len + 7) >> 3);
    for (int j = 0; j < nchunks; j++) {
        const uint64_t chunk = j == 0 ? chunk0 : load_value_chunk(col.data, begin, len, j);
        const uint64_t nb = len - 8ull * (uint64_t)j;   // valid bytes in this chunk
        const uint64_t valid = nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1);
        hit |= json_special8(chunk) & valid;
    }
    return hit == 0;
}

// byte i of a value, one cached 8-byte chunk (the escape path reads forward, at most 3 bytes ahead)
struct ValueBytes {
    const uint8_t* data;
    uint64_t begin, len;
    uint64_t k;       // chunk number held in `chunk`
    uint64_t chunk;
    __device__ __forceinline__ uint32_t at(uint64_t i) {
        if ((i >> 3) != k) {
            k = i >> 3;
            chunk = load_value_chunk(data, begin, len, (int)k);
        }
        return (uint32_t)(chunk >> (8 * (i & 7))) & 0xFFu;
    }
};

// utf8.DecodeRuneInString on the bytes at i (b0 = byte i, >= 0x80): the size of a valid sequence (2..4), 0 for RuneError of size 1
__device__ __forceinline__ uint32_t utf8_seq(ValueBytes& v, uint64_t i, uint32_t b0) {
    if (b0 < 0xC2 || b0 > 0xF4) return 0;
    const uint32_t sz = b0 < 0xE0 ? 2u : b0 < 0xF0 ? 3u : 4u;
    if (v.len - i < sz) return 0;
    const uint32_t b1 = v.at(i + 1);
    const uint32_t lo = b0 == 0xE0 ? 0xA0u : b0 == 0xF0 ? 0x90u : 0x80u;   // Go's accept ranges
    const uint32_t hi = b0 == 0xED ? 0x9Fu : b0 == 0xF4 ? 0x8Fu : 0xBFu;
    if (b1 < lo || b1 > hi) return 0;
    if (sz == 2) return 2;
    if ((v.at(i + 2) & 0xC0u) != 0x80u) return 0;
    if (sz == 3) return 3;
    return (v.at(i + 3) & 0xC0u) == 0x80u ? 4u : 0u;
}

__device__ __forceinline__ uint8_t hex_lower(uint32_t d) { return (uint8_t)(d < 10 ? '0' + d : 'a' + d - 10); }

template <class Sink>
__device__ __forceinline__ void put_bytes(Sink& s, const char* p, int n) {
    for (int q = 0; q < n; q++) s.put((uint8_t)p[q]);
}

// appendString's loop over the bytes of a value (without the surrounding quotes)
template <class Sink>
__device__ __forceinline__ void json_put_escaped(Sink& s, const uint8_t* data, uint64_t begin, uint64_t len, uint64_t chunk0) {
    ValueBytes v{data, begin, len, 0, chunk0};
    for (uint64_t i = 0; i < len;) {
        const uint32_t b = v.at(i);
        if (b < 0x80) {
            i++;
            if (b >= 0x20 && b != '"' && b != '\\') {
                s.put((uint8_t)b);
                continue;
            }
            s.put('\\');
            switch (b) {
                case '"': case '\\': s.put((uint8_t)b); break;
                case '\b': s.put('b'); break;
                case '\f': s.put('f'); break;
                case '\n': s.put('n'); break;
                case '\r': s.put('r'); break;
                case '\t': s.put('t'); break;
                default:
                    put_bytes(s, "u00", 3);
                    s.put(hex_lower(b >> 4));
                    s.put(hex_lower(b & 15));
            }
            continue;
        }
        const uint32_t sz = utf8_seq(v, i, b);
        if (sz == 0) {   // RuneError of size 1
            put_bytes(s, "\\ufffd", 6);
            i++;
            continue;
        }
        if (sz == 3 && b == 0xE2 && v.at(i + 1) == 0x80 && (v.at(i + 2) | 1u) == 0xA9) {   // U+2028, U+2029
            put_bytes(s, "\\u202", 5);
            s.put(v.at(i + 2) == 0xA8 ? '8' : '9');
        } else {
            for (uint32_t q = 0; q < sz; q++) s.put((uint8_t)v.at(i + q));
        }
        i += sz;
    }
}

// counts what a sink would receive (the length pass runs the copy pass's own escape path on the flagged fields)
struct CountSink {
    uint64_t n = 0;
    __device__ __forceinline__ void put(uint8_t) { n++; }
    __device__ __forceinline__ void put8(uint64_t, uint32_t k) { n += k; }
};

// fragment c, then the value, then its closing quote
template <class Sink>
__device__ __forceinline__ void json_put_field(Sink& s, const JsonKeys& keys, int c, const DevCol& col, uint64_t begin, uint64_t len,
                                               uint64_t chunk0, bool esc) {
    const uint64_t kb = keys.off[c], kl = keys.off[c + 1] - kb;
    for (uint64_t q = 0; q < kl; q += 8) s.put8(load_value_chunk(keys.bytes, kb, kl, (int)(q >> 3)), (uint32_t)(kl - q < 8 ? kl - q : 8));
    if (!esc) {
        for (uint64_t q = 0; q < len; q += 8) {
            const uint64_t chunk = q ? load_value_chunk(col.data, begin, len, (int)(q >> 3)) : chunk0;
            s.put8(chunk, (uint32_t)(len - q < 8 ? len - q : 8));
        }
    } else {
        json_put_escaped(s, col.data, begin, len, chunk0);
    }
    s.put('"');
}

// Record i one column at a time (a runtime loop: the escape path exists once per sink, not once per column).  The kernels
// for a fixed column count take it only for records with a field to escape, so that their common path keeps the registers
// of the CSV writer's (one escape path per column was 243 VGPRs for 6 columns).
template <class Sink>
__device__ __forceinline__ void json_put_record_rt(Sink& s, const ColsArg& cols, const ColIds& ids, int ncols, const JsonKeys& keys, uint64_t i, uint32_t flags) {
    if (i) s.put(',');
    for (int c = 0; c < ncols; c++) {
        uint64_t b, l;
        value_span(cols.c[c], source_row(ids.ids[c], i), &b, &l);
        json_put_field(s, keys, c, cols.c[c], b, l, l ? load_value_chunk(cols.c[c].data, b, l, 0) : 0, (flags >> c) & 1u);
    }
    s.put('}');
    s.put('\n');
}

// lens[i] = bytes of record i (its leading ',' included); eflags[i] bit c = field c has bytes to escape
template <int NC>
__global__ __launch_bounds__(kMatThreads) void k_json_lens(ColsArg cols, ColIds ids, int ncols, JsonKeys keys, uint64_t n,
                                                          uint64_t* __restrict__ lens, uint16_t* __restrict__ eflags) {
    const uint64_t stride = (uint64_t)gridDim.x * kMatThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kMatThreads + threadIdx.x; i < n; i += stride) {
        uint64_t total = (uint64_t)keys.fixed + (i ? 1 : 0);
        uint32_t flags = 0;
        if constexpr (NC > 0) {
            RecordFields<NC> f;
            f.load(cols, ids, i, ~0u);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                total += f.l[c];
                flags |= (uint32_t)!json_clean(cols.c[c], f.b[c], f.l[c], f.c0[c]) << c;
            }
        } else {
            for (int c = 0; c < ncols; c++) {
                uint64_t b, l;
                value_span(cols.c[c], source_row(ids.ids[c], i), &b, &l);
                total += l;
                flags |= (uint32_t)!json_clean(cols.c[c], b, l, l ? load_value_chunk(cols.c[c].data, b, l, 0) : 0) << c;
            }
        }
        // the fields to escape, one at a time: what the escape path writes beyond the raw bytes
        for (uint32_t m = flags; m; m &= m - 1) {
            const int c = __builtin_ctz(m);
            uint64_t b, l;
            value_span(cols.c[c], source_row(ids.ids[c], i), &b, &l);
            CountSink cs;
            json_put_escaped(cs, cols.c[c].data, b, l, load_value_chunk(cols.c[c].data, b, l, 0));
            total += cs.n - l;
        }
        lens[i] = total;
        eflags[i] = (uint16_t)flags;
    }
}

// out[0] = '[', record i at 1 + offs[i], out[1 + offs[n]] = ']'
template <int NC>
__global__ __launch_bounds__(kMatThreads) void k_json_copy(ColsArg cols, ColIds ids, int ncols, JsonKeys keys, uint64_t n,
                                                          const uint64_t* __restrict__ offs, const uint16_t* __restrict__ eflags,
                                                          uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    CPH_LDS uint8_t* stage = (CPH_LDS uint8_t*)smem;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // no tile writes outside [1, 1 + offs[n])
        out[0] = '[';
        out[1 + offs[n]] = ']';
    }
    for (uint64_t t0 = (uint64_t)blockIdx.x * kMatThreads; t0 < n; t0 += (uint64_t)gridDim.x * kMatThreads) {
        const uint64_t tend = t0 + kMatThreads < n ? t0 + kMatThreads : n;
        const uint64_t obase = 1 + offs[t0];
        const uint64_t span = offs[tend] - offs[t0];
        const bool staged = span + 48 <= (uint64_t)kJsonStage;   // uniform
        if (staged) {   // the words are OR-ed in: the stage starts out zero
            stage_clear(stage, span);
            __syncthreads();
        }
        const uint64_t i = t0 + threadIdx.x;
        if constexpr (NC > 0) {
            // threads past the tile's end load its last record (never written): the loads of a record stay unbranched
            RecordFields<NC> f;
            f.load(cols, ids, i < tend ? i : tend - 1, ~0u);
            if (i < tend) {
                const uint32_t flags = eflags[i];
                auto put_all = [&](auto& s) {
                    if (flags) {
                        json_put_record_rt(s, cols, ids, NC, keys, i, flags);
                        return;
                    }
                    if (i) s.put(',');
#pragma unroll
                    for (int c = 0; c < NC; c++) json_put_field(s, keys, c, cols.c[c], f.b[c], f.l[c], f.c0[c], false);
                    s.put('}');
                    s.put('\n');
                };
                if (staged) {
                    WordSink s(reinterpret_cast<uint32_t*>(smem), (uint32_t)((offs[i] - offs[t0]) + (obase & 15)));
                    put_all(s);
                    s.finish();
                } else {
                    GlobalSink s{out + 1 + offs[i]};
                    put_all(s);
                }
            }
        } else if (i < tend) {
            if (staged) {
                WordSink s(reinterpret_cast<uint32_t*>(smem), (uint32_t)((offs[i] - offs[t0]) + (obase & 15)));
                json_put_record_rt(s, cols, ids, ncols, keys, i, eflags[i]);
                s.finish();
            } else {
                GlobalSink s{out + 1 + offs[i]};
                json_put_record_rt(s, cols, ids, ncols, keys, i, eflags[i]);
            }
        }
        if (staged) {
            lds_atomics_barrier();
            flush_stage(stage, out, obase, span);
            __syncthreads();
        }
    }
}

// the host's appendString for the key fragments (tiny; the same rules as json_put_escaped)
static void json_append_escaped_host(std::string* out, const uint8_t* p, uint64_t len) {
    static const char hex[] = "0123456789abcdef";
    for (uint64_t i = 0; i < len;) {
        const uint32_t b = p[i];
        if (b < 0x80) {
            i++;
            if (b >= 0x20 && b != '"' && b != '\\') { out->push_back((char)b); continue; }
            out->push_back('\\');
            switch (b) {
                case '"': case '\\': out->push_back((char)b); break;
                case '\b': out->push_back('b'); break;
                case '\f': out->push_back('f'); break;
                case '\n': out->push_back('n'); break;
                case '\r': out->push_back('r'); break;
                case '\t': out->push_back('t'); break;
                default: out->append("u00"); out->push_back(hex[b >> 4]); out->push_back(hex[b & 15]);
            }
            continue;
        }
        uint32_t sz = 0;
        if (b >= 0xC2 && b <= 0xF4) {
            sz = b < 0xE0 ? 2u : b < 0xF0 ? 3u : 4u;
            const uint32_t lo = b == 0xE0 ? 0xA0u : b == 0xF0 ? 0x90u : 0x80u, hi = b == 0xED ? 0x9Fu : b == 0xF4 ? 0x8Fu : 0xBFu;
            if (len - i < sz || p[i + 1] < lo || p[i + 1] > hi) sz = 0;
            else if (sz >= 3 && (p[i + 2] & 0xC0u) != 0x80u) sz = 0;
            else if (sz == 4 && (p[i + 3] & 0xC0u) != 0x80u) sz = 0;
        }
        if (sz == 0) { out->append("\\ufffd"); i++; continue; }
        if (sz == 3 && b == 0xE2 && p[i + 1] == 0x80 && (p[i + 2] | 1u) == 0xA9) {
            out->append("\\u202");
            out->push_back(p[i + 2] == 0xA8 ? '8' : '9');
        } else {
            out->append(reinterpret_cast<const char*>(p + i), sz);
        }
        i += sz;
    }
}

}  // namespace cph

using namespace cph;

extern "C" {

CPH_API int32_t cph_json_write_rows(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, const cph_strval* names, int32_t ncols,
                                    uint64_t nrows, int32_t out_mem, cph_bytes** out) {
    if (!ctx || !cols || !out) return CPH_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_with(ctx, {CPH_ERR_HIP, "hipSetDevice failed"});
    *out = nullptr;
    if (!names) return fail_with(ctx, {CPH_ERR_INVALID, "cph_json_write_rows: names must not be NULL"});
    if (out_mem != CPH_MEM_HOST && out_mem != CPH_MEM_DEVICE) return fail_with(ctx, {CPH_ERR_INVALID, "bad out_mem"});
    if (ncols < 1 || ncols > CPH_MAX_KEY_COLS) return fail_with(ctx, {CPH_ERR_INVALID, "1..16 columns"});
    {
        Status s = check_row_sources(cols, sel, ncols, 0, nrows, true);
        if (!s.ok()) return fail_with(ctx, s);
    }
    for (int c = 0; c < ncols; c++)
        if (!names[c].data && names[c].len) return fail_with(ctx, {CPH_ERR_INVALID, "a name with bytes but no data pointer"});
    // map keys in byte order (sort.Strings in encoding/json's map encoder); a map holds each key once
    std::vector<std::string> key(ncols);
    for (int c = 0; c < ncols; c++) key[c].assign(reinterpret_cast<const char*>(names[c].data), (size_t)names[c].len);
    auto less = [&](int a, int b) {
        const size_t m = std::min(key[a].size(), key[b].size());
        const int r = m ? memcmp(key[a].data(), key[b].data(), m) : 0;
        return r != 0 ? r < 0 : key[a].size() < key[b].size();
    };
    std::vector<int> order(ncols);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), less);
    for (int k = 1; k < ncols; k++)
        if (key[order[k - 1]] == key[order[k]]) return fail_with(ctx, {CPH_ERR_INVALID, "cph_json_write_rows: duplicate column name"});
    const uint64_t n = nrows;
    auto* r = new (std::nothrow) cph_bytes_impl();
    if (!r) return fail_with(ctx, {CPH_ERR_NOMEM, "out of host memory"});
    r->own.ctx = ctx;
    auto run = [&]() -> Status {
        std::string frags;
        JsonKeys keys{};
        for (int k = 0; k < ncols; k++) {
            keys.off[k] = (uint32_t)frags.size();
            frags.push_back(k ? ',' : '{');
            frags.push_back('"');
            json_append_escaped_host(&frags, reinterpret_cast<const uint8_t*>(key[order[k]].data()), key[order[k]].size());
            frags.append("\":\"");
        }
        keys.off[ncols] = (uint32_t)frags.size();
        keys.fixed = (uint32_t)frags.size() + (uint32_t)ncols + 2;   // + the closing quotes + "}\n"
        std::vector<DevBuf> staged;
        ColsArg arg{};
        ColIds ids{};
        CPH_TRY(stage_row_sources(ctx, cols, sel, order.data(), ncols, 0, n, &staged, &arg, &ids));
        uint64_t total = 0;
        if (n) {
            DevBuf kbuf, offs, eflags;
            CPH_TRY(upload_block(ctx, frags.data(), frags.size(), &kbuf, 16));
            keys.bytes = kbuf.as<uint8_t>();
            CPH_TRY(offs.alloc(&ctx->pool, (n + 1) * sizeof(uint64_t)));
            CPH_TRY(eflags.alloc(&ctx->pool, (n + 1) * sizeof(uint16_t)));
            {
                ProfScope ps(ctx, "k_json_lens", 0);
                CPH_CSV_DISPATCH(k_json_lens, ncols, dim3(grid_rows(n)), 0, ctx->stream, arg, ids, ncols, keys, n, offs.as<uint64_t>(),
                                 eflags.as<uint16_t>());
            }
            CPH_HIP_TRY(hipGetLastError());
            CPH_TRY(scan_lengths(ctx, offs.as<uint64_t>(), n, &total));
            CPH_TRY(r->d_data.alloc(&ctx->pool, total + 2 + 16));
            {
                ProfScope ps(ctx, "k_json_copy", 2.0 * (double)total + 10.0 * (double)n);
                CPH_CSV_DISPATCH(k_json_copy, ncols, dim3(grid_rows(n)), kJsonStage, ctx->stream, arg, ids, ncols, keys, n, offs.as<uint64_t>(),
                                 eflags.as<uint16_t>(), r->d_data.as<uint8_t>());
            }
            CPH_HIP_TRY(hipGetLastError());
        } else {   // no rows: "[]"
            CPH_TRY(upload_block(ctx, "[]", 2, &r->d_data, 16));
        }
        r->pub.size = total + 2;
        r->pub.mem = out_mem;
        const ResultPart part{&r->d_data, (size_t)total + 2, &r->pub.data};
        return deliver(ctx, &r->own, &part, 1, out_mem);
    };
    return finish_call(ctx, r, run(), out);
}

}  // extern "C"
