// voice_cache.h — the voices a server has met: a bounded LRU map from a reference clip (its path, file size and
// modification time) to its speaker embedding.
//
// resolve() takes the reference paths of one set of requests, answers the known ones from the map, loads the others
// (each distinct file once) and hands ALL of them to the encoder in ONE call -- the batched speaker encoder
// (q3t_speaker_encode_batch) makes one launch train of them -- then stores the good embeddings and reports every path's
// failure text.  A file that changed on disk (another size or modification time) is another key: a miss.  A failed
// clip is not stored, so it is tried again when it is named again.
// The loader delivers a file's samples at the encoder's rate; the pipeline's is load_audio_file + resample_linear, the
// reference's linear resampling, so a clip named in a request gives the floats the -r flag gives.
// Header-only and free of the GPU libraries so tests/cpp/test_voice_cache.cpp drives it on the CPU.  Not thread-safe:
// one thread resolves (the one that runs the queue).
#ifndef QWEN3_TTS_VOICE_CACHE_H
#define QWEN3_TTS_VOICE_CACHE_H

#include <sys/stat.h>

#include <cstdint>
#include <functional>
#include <list>
#include <map>
#include <string>
#include <tuple>
#include <vector>

namespace qwen3_tts {

class VoiceCache {
public:
    // samples of the file at the encoder's sample rate; false: error says why
    using load_fn = std::function<bool(const std::string &path, std::vector<float> &samples, std::string &error)>;
    // all clips of one resolve: embeddings[i] for clips[i], errors[i] empty when it is good (both sized by the callee)
    using encode_fn = std::function<void(const std::vector<std::vector<float>> &clips,
                                         std::vector<std::vector<float>> &embeddings, std::vector<std::string> &errors)>;

    explicit VoiceCache(load_fn load, size_t capacity = 64) : load_(std::move(load)), capacity_(capacity ? capacity : 1) {}

    size_t size() const { return lru_.size(); }
    size_t capacity() const { return capacity_; }

    // embeddings[i] / errors[i] for paths[i] (errors[i] empty: embeddings[i] holds the voice).  encode is called at most
    // once, with the distinct files the map does not hold, in the order of their first mention
    void resolve(const std::vector<std::string> &paths, const encode_fn &encode, std::vector<std::vector<float>> &embeddings,
                 std::vector<std::string> &errors) {
        const size_t n = paths.size();
        embeddings.assign(n, {});
        errors.assign(n, "");
        std::vector<Key> keys(n);
        std::map<Key, size_t> miss;            // key -> index into clips
        std::vector<Key> miss_keys;
        std::vector<std::vector<float>> clips;
        std::map<Key, std::string> failed;     // files that did not load
        std::vector<int> from(n, -1);          // index into clips, -1: answered (hit or failure) already
        for (size_t i = 0; i < n; ++i) {
            if (!key_of(paths[i], keys[i])) { errors[i] = "Failed to load reference audio: " + paths[i]; continue; }
            auto hit = map_.find(keys[i]);
            if (hit != map_.end()) {
                lru_.splice(lru_.begin(), lru_, hit->second);   // most recently used
                embeddings[i] = hit->second->embedding;
                continue;
            }
            auto f = failed.find(keys[i]);
            if (f != failed.end()) { errors[i] = f->second; continue; }
            auto m = miss.find(keys[i]);
            if (m == miss.end()) {
                std::vector<float> samples;
                std::string why;
                if (!load_(paths[i], samples, why)) {
                    errors[i] = failed[keys[i]] = why.empty() ? "Failed to load reference audio: " + paths[i] : why;
                    continue;
                }
                m = miss.emplace(keys[i], clips.size()).first;
                miss_keys.push_back(keys[i]);
                clips.push_back(std::move(samples));
            }
            from[i] = (int)m->second;
        }
        if (clips.empty()) return;
        std::vector<std::vector<float>> emb;
        std::vector<std::string> err;
        encode(clips, emb, err);
        emb.resize(clips.size());
        err.resize(clips.size());
        for (size_t i = 0; i < n; ++i) {
            if (from[i] < 0) continue;
            if (err[from[i]].empty()) embeddings[i] = emb[from[i]];
            else errors[i] = err[from[i]];
        }
        for (size_t c = 0; c < clips.size(); ++c)
            if (err[c].empty()) store(miss_keys[c], std::move(emb[c]));
    }

private:
    using Key = std::tuple<std::string, int64_t, int64_t, int64_t>;   // path, size, mtime s, mtime ns
    struct Entry { Key key; std::vector<float> embedding; };

    static bool key_of(const std::string &path, Key &k) {
        struct stat st;
        if (path.empty() || stat(path.c_str(), &st) != 0) return false;
        k = Key(path, (int64_t)st.st_size, (int64_t)st.st_mtim.tv_sec, (int64_t)st.st_mtim.tv_nsec);
        return true;
    }
    void store(const Key &k, std::vector<float> &&e) {
        lru_.push_front(Entry{k, std::move(e)});
        map_[k] = lru_.begin();
        while (lru_.size() > capacity_) {   // the least recently used leaves
            map_.erase(lru_.back().key);
            lru_.pop_back();
        }
    }

    load_fn load_;
    size_t capacity_;
    std::list<Entry> lru_;   // front: most recently used
    std::map<Key, std::list<Entry>::iterator> map_;
};

}  // namespace qwen3_tts

#endif
