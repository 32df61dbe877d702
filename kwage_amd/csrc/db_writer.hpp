// kwage_amd/csrc/db_writer.hpp -- what the writers of a raw `.db` file share (builder.hip kwage_build_db: from `.bloom`
// files; save.hip kwage_group_save_db: from a resident group): the header as build_db() leaves it (build_db.cpp:189-199),
// the loop that takes the slice block off the device chunk of rows by chunk with its CRC32 and file write on a host
// thread, and the metadata index + records + final header behind it (build_db.cpp:371-427).
#ifndef KWAGE_AMD_DB_WRITER_HPP
#define KWAGE_AMD_DB_WRITER_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include <zlib.h>

#include "bloom_files.hpp"
#include "internal.h"

namespace kwage {

// crc32 of a large buffer continued from `crc`: parts in parallel, stitched with crc32_combine
// (the result is identical to one sequential crc32_z call).
inline uint32_t crc32_parallel(uint32_t crc, const unsigned char *buf, uint64_t len)
{
	const unsigned nthread = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
	if(len < (8u << 20) || nthread == 1){ return (uint32_t)crc32_z(crc, buf, len); }
	const uint64_t part = (len + nthread - 1)/nthread;
	std::vector<uint32_t> pc(nthread, 0);
	std::vector<uint64_t> pl(nthread, 0);
	for(unsigned t = 0; t < nthread; ++t){ pl[t] = ((uint64_t)t*part < len) ? std::min(part, len - (uint64_t)t*part) : 0; }
	run_parts(nthread, [&](unsigned t) { if(pl[t]){ pc[t] = (uint32_t)crc32_z(crc32_z(0L, Z_NULL, 0), buf + (uint64_t)t*part, pl[t]); } });
	uint64_t out = crc;
	for(unsigned t = 0; t < nthread && pl[t]; ++t){ out = crc32_combine(out, pc[t], (z_off_t)pl[t]); }
	return (uint32_t)out;
}

inline void db_put32(unsigned char *p, uint32_t v) { for(int i = 0; i < 4; ++i){ p[i] = (unsigned char)(v >> (8*i)); } }
inline void db_put64(unsigned char *p, uint64_t v) { for(int i = 0; i < 8; ++i){ p[i] = (unsigned char)(v >> (8*i)); } }

// The header of a file of n filters, kwage.h:36-46: crc32 and info_start still 0 (write_db_tail fills them in);
// hash_func stays 0 and compression NO_COMPRESSION, as build_db.cpp:189-199 leaves them.
inline void db_header_placeholder(unsigned char (&hdr)[DB_HEADER_BYTES], const kwage_params &params, uint32_t n)
{
	memset(hdr, 0, sizeof(hdr));
	db_put32(hdr, KWAGE_MAGIC_NUMBER); db_put32(hdr + 4, 2 /* CURRENT_DBFILE_VERSION */);
	db_put32(hdr + 12, params.kmer_len); db_put32(hdr + 16, params.num_hash); db_put32(hdr + 20, params.log_2_filter_len);
	db_put32(hdr + 24, n);
}

// The slice block of a file, chunk of rows by chunk, from the device to `fout`.  produce(r0, nr, ev0, ev1) queues on
// `stream` whatever leaves rows r0 .. r0 + nr - 1 of the block (nr * slice_size bytes, the file's bytes exactly) in d_out,
// with ev0 / ev1 recorded around its kernel; it returns a hipError_t.  The chunk is copied into one of two pinned blocks
// of chunk_rows * slice_size bytes, used alternately: a chunk's CRC32 and file write run on a host thread beside the next
// chunk's produce and copy.  *crc continues from its value; *io_ok turns false when a write fails (the loop stops);
// *kernel_ms: the events' durations summed; *chunks: chunks taken.
template <typename PRODUCE>
hipError_t write_db_body(FILE *fout, hipStream_t stream, uint64_t nrows, uint64_t chunk_rows, uint64_t slice_size, const void *d_out,
                         PRODUCE &&produce, uint32_t *crc, bool *io_ok, double *kernel_ms, uint32_t *chunks)
{
	void *h_out[2] = {nullptr, nullptr};
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	hipError_t e = hipSuccess;
	for(int k = 0; k < 2; ++k){ if(e == hipSuccess){ e = hipHostMalloc(&h_out[k], chunk_rows*slice_size, hipHostMallocDefault); } }
	if(e == hipSuccess){ e = hipEventCreate(&ev0); }
	if(e == hipSuccess){ e = hipEventCreate(&ev1); }
	std::thread writer;                 // CRC32 + fwrite of the previous chunk
	bool writer_ok = true;
	uint32_t n_chunk = 0;
	uint32_t db_crc = *crc;
	double t_kernel_ms = 0;
	bool ok = *io_ok;
	for(uint64_t r0 = 0; r0 < nrows && ok && e == hipSuccess; r0 += chunk_rows){
		const uint64_t nr = std::min(chunk_rows, nrows - r0);
		e = produce(r0, nr, ev0, ev1);
		unsigned char *hb = (unsigned char*)h_out[n_chunk++ & 1];      // (its previous user, two chunks ago, was joined below)
		if(e == hipSuccess){ e = hipMemcpyAsync(hb, d_out, nr*slice_size, hipMemcpyDeviceToHost, stream); }
		if(e == hipSuccess){ e = hipStreamSynchronize(stream); }
		if(e != hipSuccess){ break; }
		float ms = 0;
		(void)hipEventElapsedTime(&ms, ev0, ev1);
		t_kernel_ms += ms;
		if(writer.joinable()){ writer.join(); }
		ok = writer_ok;
		if(!ok){ break; }
		auto write_chunk = [&db_crc, &writer_ok, fout, hb, bytes = nr*slice_size]() {        // (chunks are written in order: one writer at a time)
			db_crc = crc32_parallel(db_crc, hb, bytes);
			writer_ok = fwrite(hb, 1, bytes, fout) == bytes;
		};
		try{ writer = std::thread(write_chunk); }
		catch(...){ write_chunk(); }          // no thread to be had: this chunk is written here (no exception leaves this function)
	}
	if(writer.joinable()){ writer.join(); }
	for(int k = 0; k < 2; ++k){ if(h_out[k]){ (void)hipHostFree(h_out[k]); } }
	if(ev0){ (void)hipEventDestroy(ev0); }
	if(ev1){ (void)hipEventDestroy(ev1); }
	*crc = db_crc;
	*io_ok = ok && writer_ok;
	*kernel_ms = t_kernel_ms;
	*chunks = n_chunk;
	return e;
}

// Behind the slice block: info_loc[n], the n FilterInfo records (`recs`: one after the other, rec_len[i] bytes each),
// then the header again with the CRC32 and info_start (build_db.cpp:371-427).  *db_bytes = the file's size.
inline bool write_db_tail(FILE *fout, unsigned char (&hdr)[DB_HEADER_BYTES], uint32_t crc, uint64_t info_start,
                          const std::vector<uint64_t> &rec_len, const std::vector<unsigned char> &recs, uint64_t *db_bytes)
{
	const uint64_t n = rec_len.size();
	std::vector<unsigned char> locb(8ull*n);
	uint64_t pos = info_start + 8ull*n;
	for(uint64_t i = 0; i < n; ++i){ db_put64(locb.data() + 8ull*i, pos); pos += rec_len[i]; }
	bool ok = fwrite(locb.data(), 1, locb.size(), fout) == locb.size();
	ok = ok && (recs.empty() || fwrite(recs.data(), 1, recs.size(), fout) == recs.size());
	db_put32(hdr + 8, crc);
	db_put64(hdr + 36, info_start);
	ok = ok && fseek(fout, 0, SEEK_SET) == 0 && fwrite(hdr, 1, sizeof(hdr), fout) == sizeof(hdr);
	*db_bytes = pos;
	return ok;
}

}  // namespace kwage

#endif
